// Attributes in the TSDF volume (include/ecm_color.h has the definitions): up to four planes of colour are
// integrated with the disparity maps, raycast back with them and sampled at points.  All three kernels are gathers: a thread owns
// its voxels, its pixel or its point, there are no atomics and no workgroup waits for another, so all are bit-reproducible.
//   integrate  disp_volume.hip's launch: a brick of 16 x 4 x 4 threads, VEC consecutive voxels along x per thread (VEC = 4 where
//              nx % 4 == 0 and all four operands are 16-byte aligned: one 16-byte load and store for each of the 2 + A + 1
//              planes; else 1), the view loop inside the thread.  The projection and the tsdf update are disp_volume.h's
//              integrate_view; the attribute update is the functor it calls with (pix, w, s).  A is a template parameter, so the
//              attributes of a thread are registers.
//   raycast    disp_volume.hip's launch and disp_volume.h's march; at the hit the functor blends the attributes.
//   sample     one thread per point; the matrix is uniform.
// The whole file is compiled with contraction off: every product and sum is one IEEE operation, as the header states them.
#include "disp_geom.h"
#include "disp_volume.h"
#include "../../include/ecm_color.h"

#pragma clang fp contract(off)

namespace {

using namespace ecm_vol;

constexpr int MAX_ATTRIBUTES = 4;

// ---- integrate -----------------------------------------------------------------------------------------------------------------
template <int VEC, int A>
__global__ __launch_bounds__(THREADS) void integrate_color_kernel(float* __restrict__ tsdf, float* __restrict__ wsum,
                                                                  float* __restrict__ attr, float* __restrict__ asum,
                                                                  const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                                  const float* __restrict__ weight, const float* __restrict__ attributes,
                                                                  const double* __restrict__ Q, const double* __restrict__ Gm,
                                                                  const double* __restrict__ Cm, int m_stride, int nx, int ny, int nz,
                                                                  int bx, int by, int V, int H, int W, Gates g) {
    Voxels o;
    if (!brick_voxels<VEC>(o, nx, ny, nz, bx, by)) return;
    const size_t plane = (size_t)nx * ny * nz;                              // VEC == 4: a multiple of 4, so every plane of attr is aligned
    float X[VEC], N[VEC], Y[A][VEC], Na[VEC];
    load_voxels<VEC>(X, tsdf + o.at);
    load_voxels<VEC>(N, wsum + o.at);
#pragma unroll
    for (int a = 0; a < A; ++a) load_voxels<VEC>(Y[a], attr + a * plane + o.at);
    load_voxels<VEC>(Na, asum + o.at);
    const double dj = (double)o.j, dk = (double)o.k;
    const size_t hw = (size_t)H * W;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        const double* __restrict__ G = Gm + (size_t)v * m_stride;
        const double* __restrict__ C = Cm + (size_t)v * m_stride;
        const float* __restrict__ dv = disp + v * hw;
        const unsigned char* __restrict__ vv = valid ? valid + v * hw : nullptr;
        const float* __restrict__ wv = weight ? weight + v * hw : nullptr;
        const float* __restrict__ av = attributes + (size_t)v * A * hw;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            integrate_view(X[e], N[e], (double)(o.i0 + e), dj, dk, G, C, Q, dv, vv, wv, H, W, g, [&](size_t pix, float w, double s) {
                if (!(s <= g.trunc)) return;
                float c[A];
                bool usable = true;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    c[a] = av[a * hw + pix];
                    usable = usable && ecm_finite(c[a]);
                }
                if (!usable) return;
                const float An = Na[e] + w;
#pragma unroll
                for (int a = 0; a < A; ++a) Y[a][e] = (Y[a][e] * Na[e] + c[a] * w) / An;
                Na[e] = fminf(An, g.max_weight);
            });
    }
    store_voxels<VEC>(tsdf + o.at, X);
    store_voxels<VEC>(wsum + o.at, N);
#pragma unroll
    for (int a = 0; a < A; ++a) store_voxels<VEC>(attr + a * plane + o.at, Y[a]);
    store_voxels<VEC>(asum + o.at, Na);
}

// ---- the sampling rule ---------------------------------------------------------------------------------------------------------
// the normalised blend of the A attributes about the cell, over the corners with asum > 0; +0.0 where their weights sum to 0
template <int A>
__device__ __forceinline__ void sample_cell(float (&out)[A], const float* __restrict__ attr, const float* __restrict__ asum, size_t plane,
                                            const Cell& c, int nx, int ny) {
    const size_t base = ((size_t)c.z * ny + c.y) * nx + c.x;
    const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
    const double fx[2] = {1.0 - c.qx, c.qx}, fy[2] = {1.0 - c.qy, c.qy}, fz[2] = {1.0 - c.qz, c.qz};
    double num[A], den = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) num[a] = 0.0;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const size_t at = base + dz * sz + dy * sy + dx;
                if (asum[at] > 0.f) {
                    const double b = (fz[dz] * fy[dy]) * fx[dx];
#pragma unroll
                    for (int a = 0; a < A; ++a) num[a] = num[a] + b * (double)attr[a * plane + at];
                    den = den + b;
                }
            }
#pragma unroll
    for (int a = 0; a < A; ++a) out[a] = den == 0.0 ? 0.f : (float)(num[a] / den);
}

// ---- raycast -------------------------------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(THREADS) void raycast_color_kernel(const float* __restrict__ tsdf, const float* __restrict__ wsum,
                                                                const float* __restrict__ attr, const float* __restrict__ asum,
                                                                const double* __restrict__ Rm, const double* __restrict__ Rim, int m_stride,
                                                                float* __restrict__ out, float* __restrict__ hit_weight,
                                                                float* __restrict__ colors, int nx, int ny, int nz, int H, int W,
                                                                int tiles_x, int tiles, March mr) {
    Ray r;
    if (!tile_ray(r, H, W, tiles_x, tiles)) return;
    const size_t plane = (size_t)nx * ny * nz;
    float result = 0.f, weight = 0.f, col[A];
#pragma unroll
    for (int a = 0; a < A; ++a) col[a] = 0.f;
    march_ray(result, weight, tsdf, wsum, Rm + (size_t)r.b * m_stride, Rim + (size_t)r.b * m_stride, (double)r.x, (double)r.y, nx, ny, nz,
              mr, hit_weight != nullptr, [&](double qx, double qy, double qz) {
                  sample_cell<A>(col, attr, asum, plane, cell_about(qx, qy, qz, nx, ny, nz), nx, ny);
              });
    out[r.pix] = result;
    if (hit_weight) hit_weight[r.pix] = weight;
    const size_t hw = (size_t)H * W;
    float* __restrict__ cb = colors + (size_t)r.b * A * hw + (size_t)r.y * W + (size_t)r.x;
#pragma unroll
    for (int a = 0; a < A; ++a) cb[a * hw] = col[a];
}

// ---- sample --------------------------------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(THREADS) void sample_kernel(const float* __restrict__ attr, const float* __restrict__ asum,
                                                         const double* __restrict__ Minv, const float* __restrict__ points,
                                                         float* __restrict__ out, long long N, int nx, int ny, int nz) {
    const long long n = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (n >= N) return;
    const float* __restrict__ p = points + (size_t)n * 3;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double gx = ecm_row4(Minv, x, y, z), gy = ecm_row4(Minv + 4, x, y, z), gz = ecm_row4(Minv + 8, x, y, z);
    const double tx = (double)nx - 0.5, ty = (double)ny - 0.5, tz = (double)nz - 0.5;          // exact: the dims are below 2^31
    const bool outside = !(ecm_finite(gx) && ecm_finite(gy) && ecm_finite(gz)) || gx < -0.5 || gx > tx || gy < -0.5 || gy > ty
        || gz < -0.5 || gz > tz;
    float col[A];
#pragma unroll
    for (int a = 0; a < A; ++a) col[a] = 0.f;
    if (!outside) {
        const double cx = fmin(fmax(gx, 0.0), (double)(nx - 1)), cy = fmin(fmax(gy, 0.0), (double)(ny - 1));
        const double cz = fmin(fmax(gz, 0.0), (double)(nz - 1));
        sample_cell<A>(col, attr, asum, (size_t)nx * ny * nz, cell_about(cx, cy, cz, nx, ny, nz), nx, ny);
    }
    float* __restrict__ o = out + (size_t)n * A;
#pragma unroll
    for (int a = 0; a < A; ++a) o[a] = col[a];
}

bool attributes_fit(int A) { return A >= 1 && A <= MAX_ATTRIBUTES; }

}  // namespace

extern "C" int ecmc_max_attributes(void) { return MAX_ATTRIBUTES; }

extern "C" int ecmc_integrate_fwd(float* tsdf, float* wsum, float* attr, float* asum, const float* disp, const unsigned char* valid,
                                  const float* weight, const float* attributes, const double* Q, const double* G, const double* C,
                                  int m_per_view, int nx, int ny, int nz, int A, int V, int H, int W, float trunc, float max_weight,
                                  float min_disp, float max_disp, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && attr && asum && disp && attributes && Q && G && C);
    ECM_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && V >= 1 && H >= 1 && W >= 1);
    ECM_CHECK_ARG(ecm_positive(trunc) && ecm_positive(max_weight));
    ECM_CHECK_ARG(ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(ecm_no_alias({tsdf, wsum, attr, asum}, {disp, valid, weight, attributes, Q, G, C}));
    ECM_CHECK_ARG(tsdf != wsum && tsdf != attr && tsdf != asum && wsum != attr && wsum != asum && attr != asum);
    if (!attributes_fit(A)) return ECM_EUNSUP;
    IntegratePlan p;
    if (!integrate_plan(p, nx, ny, nz, H, W, trunc, max_weight, min_disp, max_disp, {tsdf, wsum, attr, asum})) return ECM_EUNSUP;
    return ecm_dispatch<1, 4>(p.vec, [&](auto vec) {
        return ecm_dispatch<1, 2, 3, 4>(A, [&](auto planes) {
            hipLaunchKernelGGL((integrate_color_kernel<decltype(vec)::value, decltype(planes)::value>), dim3(p.groups), dim3(THREADS), 0,
                               ecm_stream(stream), tsdf, wsum, attr, asum, disp, valid, weight, attributes, Q, G, C,
                               ecm_mat_stride(m_per_view), nx, ny, nz, (int)p.bricks.bx, (int)p.bricks.by, V, H, W, p.gates);
            return ECM_LAUNCH_RESULT();
        });
    });
}

extern "C" int ecmc_raycast_fwd(const float* tsdf, const float* wsum, const float* attr, const float* asum, const double* R,
                                const double* Rinv, int m_per_view, float* out, float* hit_weight, float* colors, int nx, int ny, int nz,
                                int A, int B, int H, int W, float near_disp, float far_disp, float step, int max_steps, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && attr && asum && R && Rinv && out && colors);
    ECM_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2 && B >= 1 && H >= 1 && W >= 1 && max_steps >= 1);
    ECM_CHECK_ARG(ecm_positive(step) && ecm_positive(far_disp) && std::isfinite(near_disp) && near_disp > far_disp);
    ECM_CHECK_ARG(ecm_no_alias({out, hit_weight, colors}, {tsdf, wsum, attr, asum, R, Rinv}));
    ECM_CHECK_ARG(out != hit_weight && out != colors && hit_weight != colors);
    if (!attributes_fit(A)) return ECM_EUNSUP;
    RayPlan p;
    if (!ray_plan(p, nx, ny, nz, B, H, W, near_disp, far_disp, step, max_steps)) return ECM_EUNSUP;
    return ecm_dispatch<1, 2, 3, 4>(A, [&](auto planes) {
        hipLaunchKernelGGL(raycast_color_kernel<decltype(planes)::value>, dim3(p.groups), dim3(THREADS), 0, ecm_stream(stream), tsdf, wsum,
                           attr, asum, R, Rinv, ecm_mat_stride(m_per_view), out, hit_weight, colors, nx, ny, nz, H, W, (int)p.tiles.x,
                           (int)p.tiles.per_view, p.march);
        return ECM_LAUNCH_RESULT();
    });
}

extern "C" int ecmc_sample_fwd(const float* attr, const float* asum, const double* Minv, const float* points, float* out, long long N,
                               int nx, int ny, int nz, int A, void* stream) {
    ECM_CHECK_ARG(attr && asum && Minv && points && out);
    ECM_CHECK_ARG(N >= 1 && nx >= 2 && ny >= 2 && nz >= 2);
    ECM_CHECK_ARG(ecm_no_alias({out}, {attr, asum, Minv, points}));
    if (!attributes_fit(A)) return ECM_EUNSUP;
    if (N > INT_MAX || (long long)nx * ny > INT_MAX || !voxels_fit(nx, ny, nz)) return ECM_EUNSUP;
    const unsigned groups = (unsigned)((N + THREADS - 1) / THREADS);        // at most 2^23
    return ecm_dispatch<1, 2, 3, 4>(A, [&](auto planes) {
        hipLaunchKernelGGL(sample_kernel<decltype(planes)::value>, dim3(groups), dim3(THREADS), 0, ecm_stream(stream), attr, asum, Minv,
                           points, out, N, nx, ny, nz);
        return ECM_LAUNCH_RESULT();
    });
}
