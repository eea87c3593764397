// The TSDF volume (include/ecm_volume.h has the definitions): disparity maps are integrated into a dense
// grid of truncated signed distances, view after view, and the grid is raycast back into a disparity map from any pose.  Both
// kernels are gathers: a thread owns its voxels or its pixel, nothing is scattered, there are no atomics and no workgroup waits
// for another, so both are bit-reproducible.
//   integrate  a workgroup of 256 owns a brick of 16 x 4 x 4 threads (x fastest); a thread owns VEC consecutive voxels along x
//              (VEC = 4 where nx % 4 == 0 and the planes are 16-byte aligned: one 16-byte load and store per plane; else 1).  The
//              view loop runs inside the thread: the voxel is read once, updated in registers and written once.  The matrices
//              are indexed by the view alone, which is uniform: the compiler keeps them in scalar registers.
//   raycast    a workgroup of 256 owns a tile of 16 x 16 pixels of one view, each wave 8 x 8 of them, so that the rays of a wave
//              pass through neighbouring cells; the two matrices are uniform per workgroup.  The march is clipped to the samples
//              that can lie inside the volume's box (a slab test with a margin of one sample on either side); every sample in
//              between is visited.
// The whole file is compiled with contraction off: every product and sum is one IEEE operation, as the header states them.
#include "disp_geom.h"
#include "../../include/ecm_volume.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int BRICK_X = 16, BRICK_Y = 4, BRICK_Z = 4;     // threads of a brick; BRICK_X * VEC voxels along x
constexpr int TILE = 16;                                  // pixels of a raycast tile, each way
constexpr int MAX_GROUPS = 16777215;                      // workgroups of a launch: its global size stays below 2^32
constexpr int MAX_STEPS = 65536;

struct Gates {
    DispRange range;
    float max_weight;
    double trunc;
};

// ---- integrate -----------------------------------------------------------------------------------------------------------------
// one view's update of one voxel: X = tsdf, N = wsum
__device__ __forceinline__ void integrate_view(float& X, float& N, double di, double dj, double dk, const double* __restrict__ G,
                                               const double* __restrict__ Cm, const double* __restrict__ Q,
                                               const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                               const float* __restrict__ weight, int H, int W, const Gates& g) {
    const double h3 = ecm_row4(G + 12, di, dj, dk);
    const double u = ecm_row4(G, di, dj, dk) / h3, v = ecm_row4(G + 4, di, dj, dk) / h3, dv = ecm_row4(G + 8, di, dj, dk) / h3;
    if (!(ecm_finite(u) && ecm_finite(v) && ecm_finite(dv) && dv > 0.0)) return;
    const double fx = floor(u + 0.5), fy = floor(v + 0.5);
    if (!(fx >= 0.0 && fx <= (double)(W - 1) && fy >= 0.0 && fy <= (double)(H - 1))) return;
    const size_t pix = (size_t)(int)fy * W + (int)fx;                       // 0 <= pix < H * W
    const float d = disp[pix];
    if (!ecm_disp_usable(d, !valid || valid[pix] != 0, g.range)) return;
    const float w = weight ? weight[pix] : 1.f;
    if (!(w > 0.f && w < __builtin_inff())) return;
    const double fd = (double)d;
    const double P3 = ecm_row4(Q + 12, fx, fy, fd);
    if (!ecm_nonzero_finite(P3)) return;
    const double z_meas = ecm_row4(Q + 8, fx, fy, fd) / P3;
    const double z_vox = ecm_row4(Cm + 8, di, dj, dk);
    if (!(ecm_finite(z_meas) && z_meas > 0.0 && ecm_finite(z_vox) && z_vox > 0.0)) return;
    const double s = z_meas - z_vox;
    if (s < -g.trunc) return;
    const float t = (float)fmin(1.0, s / g.trunc);
    const float Wn = N + w;
    X = (X * N + t * w) / Wn;
    N = fminf(Wn, g.max_weight);
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void integrate_kernel(float* __restrict__ tsdf, float* __restrict__ wsum,
                                                            const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                            const float* __restrict__ weight, const double* __restrict__ Q,
                                                            const double* __restrict__ Gm, const double* __restrict__ Cm, int m_stride,
                                                            int nx, int ny, int nz, int bx, int by, int V, int H, int W, Gates g) {
    const unsigned blk = blockIdx.x;
    const int bi = (int)(blk % (unsigned)bx), bj = (int)((blk / (unsigned)bx) % (unsigned)by), bk = (int)(blk / ((unsigned)bx * (unsigned)by));
    const int tx = threadIdx.x & (BRICK_X - 1), ty = (threadIdx.x / BRICK_X) & (BRICK_Y - 1), tz = threadIdx.x / (BRICK_X * BRICK_Y);
    const long long i0 = ((long long)bi * BRICK_X + tx) * VEC;             // bx * BRICK_X * VEC may pass nx by a brick: below 2^32
    const int j = bj * BRICK_Y + ty, k = bk * BRICK_Z + tz;
    if (i0 >= nx || j >= ny || k >= nz) return;                             // VEC == 4: nx % 4 == 0, so i0 + 3 < nx as well
    const size_t at = ((size_t)k * ny + j) * nx + (size_t)i0;               // below nx * ny * nz < 2^31

    float X[VEC], N[VEC];
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(tsdf + at), b = *reinterpret_cast<const float4*>(wsum + at);
        X[0] = a.x, X[1] = a.y, X[2] = a.z, X[3] = a.w;
        N[0] = b.x, N[1] = b.y, N[2] = b.z, N[3] = b.w;
    } else {
        X[0] = tsdf[at];
        N[0] = wsum[at];
    }
    const double dj = (double)j, dk = (double)k;
    const size_t hw = (size_t)H * W;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        const double* __restrict__ G = Gm + (size_t)v * m_stride;
        const double* __restrict__ C = Cm + (size_t)v * m_stride;
        const float* __restrict__ dv = disp + v * hw;
        const unsigned char* __restrict__ vv = valid ? valid + v * hw : nullptr;
        const float* __restrict__ wv = weight ? weight + v * hw : nullptr;
#pragma unroll
        for (int e = 0; e < VEC; ++e) integrate_view(X[e], N[e], (double)(i0 + e), dj, dk, G, C, Q, dv, vv, wv, H, W, g);
    }
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(tsdf + at) = make_float4(X[0], X[1], X[2], X[3]);
        *reinterpret_cast<float4*>(wsum + at) = make_float4(N[0], N[1], N[2], N[3]);
    } else {
        tsdf[at] = X[0];
        wsum[at] = N[0];
    }
}

// ---- raycast -------------------------------------------------------------------------------------------------------------------
struct Cell {
    int x, y, z;                              // the lower corner
    double qx, qy, qz;                        // the position within the cell
};

// the header's blend of the eight values of `plane` about the cell, widened
__device__ __forceinline__ double blend(const float* __restrict__ plane, const Cell& c, int nx, int ny) {
    const float* __restrict__ p = plane + ((size_t)c.z * ny + c.y) * nx + c.x;
    const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
    const double t000 = p[0], t001 = p[1], t010 = p[sy], t011 = p[sy + 1];
    const double t100 = p[sz], t101 = p[sz + 1], t110 = p[sz + sy], t111 = p[sz + sy + 1];
    const double a00 = t000 + c.qx * (t001 - t000), a01 = t010 + c.qx * (t011 - t010);
    const double a10 = t100 + c.qx * (t101 - t100), a11 = t110 + c.qx * (t111 - t110);
    const double e0 = a00 + c.qy * (a01 - a00), e1 = a10 + c.qy * (a11 - a10);
    return e0 + c.qz * (e1 - e0);
}

__device__ __forceinline__ bool all_weighted(const float* __restrict__ wsum, const Cell& c, int nx, int ny) {
    const float* __restrict__ p = wsum + ((size_t)c.z * ny + c.y) * nx + c.x;
    const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
    return p[0] > 0.f && p[1] > 0.f && p[sy] > 0.f && p[sy + 1] > 0.f && p[sz] > 0.f && p[sz + 1] > 0.f && p[sz + sy] > 0.f
        && p[sz + sy + 1] > 0.f;
}

// narrow [s_lo, s_hi] to where gn + dir * s can lie in [0, top) on one axis; false: it lies there for no s.  A direction too
// small for the margin of one sample to cover the rounding of a sample's own position gives no constraint at all.
__device__ __forceinline__ bool clip_axis(double gn, double dir, double top, double& s_lo, double& s_hi) {
    if (dir == 0.0) return gn >= 0.0 && gn < top;                           // every sample is gn itself
    if (!(fabs(dir) * 1073741824.0 > fabs(gn) + top)) return true;
    const double s0 = (0.0 - gn) / dir, s1 = (top - gn) / dir;
    s_lo = fmax(s_lo, fmin(s0, s1));
    s_hi = fmin(s_hi, fmax(s0, s1));
    return true;
}

__global__ __launch_bounds__(THREADS) void raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ wsum,
                                                          const double* __restrict__ Rm, const double* __restrict__ Rim, int m_stride,
                                                          float* __restrict__ out, float* __restrict__ hit_weight, int nx, int ny,
                                                          int nz, int H, int W, int tiles_x, int tiles, double near_disp,
                                                          double far_disp, double step, int max_steps) {
    const int b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long x = (long long)(tile % tiles_x) * TILE + (wave & 1) * 8 + (lane & 7);
    const long long y = (long long)(tile / tiles_x) * TILE + (wave >> 1) * 8 + (lane >> 3);
    if (x >= W || y >= H) return;
    const double* __restrict__ R = Rm + (size_t)b * m_stride;
    const double* __restrict__ Ri = Rim + (size_t)b * m_stride;
    const size_t pix = (size_t)b * H * W + (size_t)y * W + (size_t)x;
    const double fx = (double)x, fy = (double)y;

    float result = 0.f, weight = 0.f;
    const double hn = ecm_row4(R + 12, fx, fy, near_disp), hf = ecm_row4(R + 12, fx, fy, far_disp);
    const double gx = ecm_row4(R, fx, fy, near_disp) / hn, gy = ecm_row4(R + 4, fx, fy, near_disp) / hn, gz = ecm_row4(R + 8, fx, fy, near_disp) / hn;
    const double ex = ecm_row4(R, fx, fy, far_disp) / hf, ey = ecm_row4(R + 4, fx, fy, far_disp) / hf, ez = ecm_row4(R + 8, fx, fy, far_disp) / hf;
    const double dx = ex - gx, dy = ey - gy, dz = ez - gz;
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    const double nd = ceil(len / step);
    const bool ends = ecm_finite(gx) && ecm_finite(gy) && ecm_finite(gz) && ecm_finite(ex) && ecm_finite(ey) && ecm_finite(ez);
    if (ends && nd >= 1.0 && nd <= (double)max_steps) {                     // a NaN fails both comparisons
        const int n = (int)nd;
        double s_lo = 0.0, s_hi = 1.0;
        bool some = clip_axis(gx, dx, (double)(nx - 1), s_lo, s_hi) && clip_axis(gy, dy, (double)(ny - 1), s_lo, s_hi)
            && clip_axis(gz, dz, (double)(nz - 1), s_lo, s_hi);
        some = some && s_lo <= s_hi + 2.0 / nd;                             // so both are finite: -2/n <= s_hi, s_lo <= 1 + 2/n
        int m_lo = 0, m_hi = -1;
        if (some) {
            m_lo = max((int)floor(s_lo * nd) - 1, 0);
            m_hi = min((int)ceil(s_hi * nd) + 1, n);
        }
        bool before = false;                                                // the sample before this one was valid
        double f0 = 0.0, px0 = 0.0, py0 = 0.0, pz0 = 0.0;
#pragma unroll 1
        for (int m = m_lo; m <= m_hi; ++m) {
            const double s = (double)m / nd;
            const double px = gx + dx * s, py = gy + dy * s, pz = gz + dz * s;
            const double cx = floor(px), cy = floor(py), cz = floor(pz);
            bool ok = cx >= 0.0 && cx <= (double)(nx - 2) && cy >= 0.0 && cy <= (double)(ny - 2) && cz >= 0.0 && cz <= (double)(nz - 2);
            double f = 0.0;
            if (ok) {
                const Cell c = {(int)cx, (int)cy, (int)cz, px - cx, py - cy, pz - cz};
                ok = all_weighted(wsum, c, nx, ny);
                if (ok) f = blend(tsdf, c, nx, ny);
            }
            if (ok && before) {
                if (f0 > 0.0 && f <= 0.0) {
                    const double a = f0 / (f0 - f);
                    const double qx = px0 + (px - px0) * a, qy = py0 + (py - py0) * a, qz = pz0 + (pz - pz0) * a;
                    result = (float)(ecm_row4(Ri + 8, qx, qy, qz) / ecm_row4(Ri + 12, qx, qy, qz));
                    if (hit_weight) {
                        const double wx = fmin(fmax(floor(qx), 0.0), (double)(nx - 2)), wy = fmin(fmax(floor(qy), 0.0), (double)(ny - 2));
                        const double wz = fmin(fmax(floor(qz), 0.0), (double)(nz - 2));
                        const Cell c = {(int)wx, (int)wy, (int)wz, qx - wx, qy - wy, qz - wz};
                        weight = (float)blend(wsum, c, nx, ny);
                    }
                    break;
                }
                if (f0 < 0.0 && f > 0.0) break;                             // a back face
            }
            before = ok;
            f0 = f, px0 = px, py0 = py, pz0 = pz;
        }
    }
    out[pix] = result;
    if (hit_weight) hit_weight[pix] = weight;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
bool voxels_fit(int nx, int ny, int nz) { return (long long)nx * ny * nz <= INT_MAX; }   // after nx, ny, nz >= 1: nx * ny <= 2^62

}  // namespace

extern "C" int ecmv_integrate_fwd(float* tsdf, float* wsum, const float* disp, const unsigned char* valid, const float* weight,
                                  const double* Q, const double* G, const double* C, int m_per_view, int nx, int ny, int nz, int V,
                                  int H, int W, float trunc, float max_weight, float min_disp, float max_disp, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && disp && Q && G && C);
    ECM_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && V >= 1 && H >= 1 && W >= 1);
    ECM_CHECK_ARG(ecm_positive(trunc) && ecm_positive(max_weight));
    ECM_CHECK_ARG(ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(ecm_no_alias({tsdf, wsum}, {disp, valid, weight, Q, G, C}) && tsdf != wsum);
    if ((long long)nx * ny > INT_MAX || !voxels_fit(nx, ny, nz) || (long long)H * W > INT_MAX) return ECM_EUNSUP;
    const bool wide = nx % 4 == 0 && ((uintptr_t)tsdf | (uintptr_t)wsum) % 16 == 0;
    const long long per = (long long)BRICK_X * (wide ? 4 : 1);
    const long long bx = (nx + per - 1) / per, by = (ny + BRICK_Y - 1) / BRICK_Y, bz = (nz + BRICK_Z - 1) / BRICK_Z;
    if (bx * by * bz > MAX_GROUPS) return ECM_EUNSUP;
    const Gates g = {{min_disp, max_disp}, max_weight, (double)trunc};
    const dim3 grid((unsigned)(bx * by * bz));
    return ecm_dispatch<1, 4>(wide ? 4 : 1, [&](auto vec) {
        hipLaunchKernelGGL(integrate_kernel<decltype(vec)::value>, grid, dim3(THREADS), 0, ecm_stream(stream), tsdf, wsum, disp, valid,
                           weight, Q, G, C, ecm_mat_stride(m_per_view), nx, ny, nz, (int)bx, (int)by, V, H, W, g);
        return ECM_LAUNCH_RESULT();
    });
}

extern "C" int ecmv_raycast_max_steps(void) { return MAX_STEPS; }

extern "C" int ecmv_raycast_fwd(const float* tsdf, const float* wsum, const double* R, const double* Rinv, int m_per_view, float* out,
                                float* hit_weight, int nx, int ny, int nz, int B, int H, int W, float near_disp, float far_disp,
                                float step, int max_steps, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && R && Rinv && out);
    ECM_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2 && B >= 1 && H >= 1 && W >= 1 && max_steps >= 1);
    ECM_CHECK_ARG(ecm_positive(step) && ecm_positive(far_disp) && std::isfinite(near_disp) && near_disp > far_disp);
    ECM_CHECK_ARG(ecm_no_alias({out, hit_weight}, {tsdf, wsum, R, Rinv}) && out != hit_weight);
    if ((long long)nx * ny > INT_MAX || !voxels_fit(nx, ny, nz) || (long long)H * W > INT_MAX) return ECM_EUNSUP;
    if (max_steps > MAX_STEPS) return ECM_EUNSUP;
    const long long tiles_x = ((long long)W + TILE - 1) / TILE, tiles_y = ((long long)H + TILE - 1) / TILE;
    if (tiles_x * tiles_y * B > MAX_GROUPS) return ECM_EUNSUP;
    hipLaunchKernelGGL(raycast_kernel, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(THREADS), 0, ecm_stream(stream), tsdf, wsum, R, Rinv,
                       ecm_mat_stride(m_per_view), out, hit_weight, nx, ny, nz, H, W, (int)tiles_x, (int)(tiles_x * tiles_y), (double)near_disp,
                       (double)far_disp, (double)step, max_steps);
    return ECM_LAUNCH_RESULT();
}
