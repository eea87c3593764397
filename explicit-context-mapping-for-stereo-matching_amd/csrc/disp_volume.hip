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
// The per-voxel update and the march themselves are in disp_volume.h, which disp_color.hip shares.
// The whole file is compiled with contraction off: every product and sum is one IEEE operation, as the header states them.
#include "disp_geom.h"
#include "disp_volume.h"
#include "../../include/ecm_volume.h"

#pragma clang fp contract(off)

namespace {

using namespace ecm_vol;

// ---- integrate -----------------------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(THREADS) void integrate_kernel(float* __restrict__ tsdf, float* __restrict__ wsum,
                                                            const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                            const float* __restrict__ weight, const double* __restrict__ Q,
                                                            const double* __restrict__ Gm, const double* __restrict__ Cm, int m_stride,
                                                            int nx, int ny, int nz, int bx, int by, int V, int H, int W, Gates g) {
    Voxels o;
    if (!brick_voxels<VEC>(o, nx, ny, nz, bx, by)) return;
    float X[VEC], N[VEC];
    load_voxels<VEC>(X, tsdf + o.at);
    load_voxels<VEC>(N, wsum + o.at);
    const double dj = (double)o.j, dk = (double)o.k;
    const size_t hw = (size_t)H * W;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        const double* __restrict__ G = Gm + (size_t)v * m_stride;
        const double* __restrict__ C = Cm + (size_t)v * m_stride;
        const float* __restrict__ dv = disp + v * hw;
        const unsigned char* __restrict__ vv = valid ? valid + v * hw : nullptr;
        const float* __restrict__ wv = weight ? weight + v * hw : nullptr;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            integrate_view(X[e], N[e], (double)(o.i0 + e), dj, dk, G, C, Q, dv, vv, wv, H, W, g, [](size_t, float, double) {});
    }
    store_voxels<VEC>(tsdf + o.at, X);
    store_voxels<VEC>(wsum + o.at, N);
}

// ---- raycast -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ wsum,
                                                          const double* __restrict__ Rm, const double* __restrict__ Rim, int m_stride,
                                                          float* __restrict__ out, float* __restrict__ hit_weight, int nx, int ny,
                                                          int nz, int H, int W, int tiles_x, int tiles, March mr) {
    Ray r;
    if (!tile_ray(r, H, W, tiles_x, tiles)) return;
    float result = 0.f, weight = 0.f;
    march_ray(result, weight, tsdf, wsum, Rm + (size_t)r.b * m_stride, Rim + (size_t)r.b * m_stride, (double)r.x, (double)r.y, nx, ny, nz,
              mr, hit_weight != nullptr, [](double, double, double) {});
    out[r.pix] = result;
    if (hit_weight) hit_weight[r.pix] = weight;
}

}  // namespace

extern "C" int ecmv_integrate_fwd(float* tsdf, float* wsum, const float* disp, const unsigned char* valid, const float* weight,
                                  const double* Q, const double* G, const double* C, int m_per_view, int nx, int ny, int nz, int V,
                                  int H, int W, float trunc, float max_weight, float min_disp, float max_disp, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && disp && Q && G && C);
    ECM_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && V >= 1 && H >= 1 && W >= 1);
    ECM_CHECK_ARG(ecm_positive(trunc) && ecm_positive(max_weight));
    ECM_CHECK_ARG(ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(ecm_no_alias({tsdf, wsum}, {disp, valid, weight, Q, G, C}) && tsdf != wsum);
    IntegratePlan p;
    if (!integrate_plan(p, nx, ny, nz, H, W, trunc, max_weight, min_disp, max_disp, {tsdf, wsum})) return ECM_EUNSUP;
    return ecm_dispatch<1, 4>(p.vec, [&](auto vec) {
        hipLaunchKernelGGL(integrate_kernel<decltype(vec)::value>, dim3(p.groups), dim3(THREADS), 0, ecm_stream(stream), tsdf, wsum, disp,
                           valid, weight, Q, G, C, ecm_mat_stride(m_per_view), nx, ny, nz, (int)p.bricks.bx, (int)p.bricks.by, V, H, W,
                           p.gates);
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
    RayPlan p;
    if (!ray_plan(p, nx, ny, nz, B, H, W, near_disp, far_disp, step, max_steps)) return ECM_EUNSUP;
    hipLaunchKernelGGL(raycast_kernel, dim3(p.groups), dim3(THREADS), 0, ecm_stream(stream), tsdf, wsum, R, Rinv,
                       ecm_mat_stride(m_per_view), out, hit_weight, nx, ny, nz, H, W, (int)p.tiles.x, (int)p.tiles.per_view, p.march);
    return ECM_LAUNCH_RESULT();
}
