// Temporal carry of a disparity map (include/ecm_temporal.h has the definitions): the z-buffered forward warp
// of a disparity map by a 4x4 fp64 matrix M = Q_out^-1 T Q -- a 2-D scatter, where disp_splat.hip stays inside a row and inside
// LDS -- and the per-pixel fusion of the warped state with the next frame's own estimate.
// A workgroup owns one linear pixel tile (disp_geom.h): M is uniform per workgroup.
//   clear    hipMemsetAsync of the keys, one 8-byte word per pixel of the batch;
//   scatter  every pixel: the usable rule, [a b c w] = M [x y d 1] in fp64, the candidate rule, the 64-bit key (the bits of the new
//            disparity above the source's linear index), and an integer atomic max of it on each of its one to four landing
//            sites in global memory.  The result of the atomic is not used: nothing waits for it;
//   resolve  every pixel: its key read coalesced, decoded; the attribute planes gathered at the winner's source; out, src and
//            attrs_out stored.
//   fuse     one elementwise launch: the scalar Kalman update of include/ecm_temporal.h, fp32 in the stated order.
// The only atomics are integer maxima and no workgroup waits for another (the rule disp_speckle.hip states): the result does not
// depend on the order of arrival and is bit-reproducible.  No LDS, no scratch memory.
#include "disp_geom.h"
#include "../../include/ecm_temporal.h"

namespace {

using namespace ecm_pix;
constexpr int MAX_ATTRS = 4;
constexpr int FUSE_GRID = 4096;               // workgroups of the fusion launch at most; each walks elements a grid apart

typedef unsigned long long u64;

// ---- scatter -----------------------------------------------------------------------------------------------------------------
template <int NEAREST>
__global__ __launch_bounds__(THREADS) void warp_scatter(const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                        const double* __restrict__ M, int m_stride, u64* __restrict__ keys, int HW,
                                                        int W, int H, int T, DispRange r) {
    const PixTile t = ecm_pix_tile(T);
    const double* m = M + (size_t)t.b * m_stride;
    const size_t img = (size_t)t.b * HW;
    u64* best = keys + img;
    const double last_x = (double)(W - 1), last_y = (double)(H - 1);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned pix = t.first + k * THREADS + threadIdx.x;
        if (pix >= (unsigned)HW) continue;
        const float d = disp[img + pix];
        if (!ecm_disp_usable(d, !valid || valid[img + pix] != 0, r)) continue;
        int x, y;
        ecm_pix_xy(pix, W, x, y);
        const double fx = (double)x, fy = (double)y, fd = (double)d;
        const double w = ecm_row4(m + 12, fx, fy, fd);
        if (!ecm_nonzero_finite(w)) continue;
        const double u = ecm_row4(m, fx, fy, fd) / w, vv = ecm_row4(m + 4, fx, fy, fd) / w;
        const float dn = (float)(ecm_row4(m + 8, fx, fy, fd) / w);
        // every comparison fails on a NaN; u and vv inside the image are finite
        if (!(fabsf(dn) < __builtin_inff() && dn > 0.f && u >= 0.0 && u <= last_x && vv >= 0.0 && vv <= last_y)) continue;
        const u64 key = ((u64)__float_as_uint(dn) << 32) | (u64)pix;
        if (NEAREST) {
            const int xn = min((int)floor(u + 0.5), W - 1), yn = min((int)floor(vv + 0.5), H - 1);
            atomicMax(&best[(size_t)yn * W + xn], key);
        } else {
            const double fu = floor(u), fv = floor(vv);
            const int x0 = (int)fu, y0 = (int)fv;                          // 0 <= x0 <= W-1, 0 <= y0 <= H-1
            const bool right = u > fu, down = vv > fv;
            const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);     // u > fu implies x0 < W-1; the min keeps the bound explicit
            atomicMax(&best[(size_t)y0 * W + x0], key);
            if (right) atomicMax(&best[(size_t)y0 * W + x1], key);
            if (down) atomicMax(&best[(size_t)y1 * W + x0], key);
            if (right && down) atomicMax(&best[(size_t)y1 * W + x1], key);
        }
    }
}

// ---- resolve -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void warp_resolve(const u64* __restrict__ keys, const float* __restrict__ attrs, int C,
                                                        float* __restrict__ out, int* __restrict__ src,
                                                        float* __restrict__ attrs_out, int HW, int T) {
    const PixTile t = ecm_pix_tile(T);
    const size_t img = (size_t)t.b * HW;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned pix = t.first + k * THREADS + threadIdx.x;
        if (pix >= (unsigned)HW) continue;
        const u64 key = keys[img + pix];
        const unsigned from = (unsigned)key;                               // < HW for every key that a candidate wrote
        out[img + pix] = key ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
        if (src) src[img + pix] = key ? (int)from : -1;
        for (int a = 0; a < C; ++a) {
            const size_t plane = ((size_t)t.b * C + a) * HW;
            attrs_out[plane + pix] = key ? attrs[plane + from] : 0.f;
        }
    }
}

// ---- fuse --------------------------------------------------------------------------------------------------------------------
// not __restrict__: an output may be the input of the same type (each thread reads its element before it writes it)
__global__ __launch_bounds__(THREADS) void fuse_fwd(const float* disp, const float* var, const float* prev, const float* prev_var,
                                                    const int* prev_age, const float* prev_source, float* fused, float* fused_var,
                                                    int* age, long long n, float gate, float q, int coast) {
#pragma clang fp contract(off)
    const float inf = __builtin_inff();
    const float g2 = gate * gate;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const float d = disp[i], vr = var[i], p = prev[i], pv = prev_var[i];
        const int pa = prev_age ? prev_age[i] : 0;
        const bool meas = fabsf(d) < inf && d > 0.f && fabsf(vr) < inf && vr > 0.f;
        const bool pred = p > 0.f && fabsf(pv) < inf && pv > 0.f;
        float s = pv + q;
        if (prev_source) {
            const float r = p / prev_source[i];
            s = (((pv * r) * r) * r) * r + q;
        }
        float f = 0.f, fv = 0.f;
        int a = 0;
        if (meas) {
            const float e = d - p, sum = s + vr;
            if (pred && e * e <= g2 * sum) {
                const float K = s / sum;
                f = p + K * e;
                fv = (1.f - K) * s;
                a = pa + 1;
            } else {
                f = d;
                fv = vr;
                a = 1;
            }
        } else if (pred && coast) {
            f = p;
            fv = s;
            a = pa;
        }
        fused[i] = f;
        fused_var[i] = fv;
        age[i] = a;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// tiles per image, or 0 where the shape is refused (code: why)
int tiles_per_image(int B, int H, int W, int& code) {
    code = ECM_EINVAL;
    if (B < 1 || H < 1 || W < 1) return 0;
    code = ECM_EUNSUP;
    const long long hw = (long long)H * W;
    if (hw > INT_MAX) return 0;               // the image, not the batch: a key holds an index into the image
    return ecm_pix_tiles(hw, B, code);
}

}  // namespace

extern "C" int ecmt_disparity_warp_max_attributes(void) { return MAX_ATTRS; }

extern "C" long long ecmt_disparity_warp_scratch_bytes(int B, int H, int W) {
    int code;
    const int T = tiles_per_image(B, H, W, code);
    return T ? (long long)B * H * W * (long long)sizeof(u64) : 0;
}

extern "C" int ecmt_disparity_warp_fwd(const float* disp, const unsigned char* valid, const double* M, int m_per_image,
                                       const float* attrs, int C, float* out, int* src, float* attrs_out, void* scratch,
                                       long long scratch_bytes, int B, int H, int W, float min_disp, float max_disp, int footprint,
                                       void* stream) {
    ECM_CHECK_ARG(disp && M && out && scratch && ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(C >= 0 && C <= MAX_ATTRS && (C == 0 || (attrs && attrs_out)));
    ECM_CHECK_ARG(ecm_no_alias({out, src, C ? attrs_out : nullptr, scratch}, {disp, valid, M, C ? attrs : nullptr}));
    int code;
    const int T = tiles_per_image(B, H, W, code);
    if (!T) return code;
    if (footprint != 0 && footprint != 1) return ECM_EUNSUP;
    const long long need = ecmt_disparity_warp_scratch_bytes(B, H, W);
    if (scratch_bytes < need) return ECM_ESCRATCH;
    const DispRange r = {min_disp, max_disp};
    const int HW = H * W, m_stride = ecm_mat_stride(m_per_image), n = B * T;
    u64* keys = static_cast<u64*>(scratch);
    hipStream_t s = ecm_stream(stream);
    const hipError_t cleared = hipMemsetAsync(keys, 0, (size_t)need, s);
    if (cleared != hipSuccess) return (int)cleared;
    if (footprint)
        hipLaunchKernelGGL(warp_scatter<1>, dim3(n), dim3(THREADS), 0, s, disp, valid, M, m_stride, keys, HW, W, H, T, r);
    else
        hipLaunchKernelGGL(warp_scatter<0>, dim3(n), dim3(THREADS), 0, s, disp, valid, M, m_stride, keys, HW, W, H, T, r);
    hipLaunchKernelGGL(warp_resolve, dim3(n), dim3(THREADS), 0, s, (const u64*)keys, attrs, C, out, src, attrs_out, HW, T);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecmt_disparity_fuse_fwd(const float* disp, const float* var, const float* prev, const float* prev_var,
                                       const int* prev_age, const float* prev_source, float* fused, float* fused_var, int* age,
                                       long long n, float gate, float process_noise, int coast, void* stream) {
    ECM_CHECK_ARG(disp && var && prev && prev_var && fused && fused_var && age && n > 0);
    ECM_CHECK_ARG(std::isfinite(gate) && gate >= 0.f && std::isfinite(process_noise) && process_noise >= 0.f);
    const long long blocks = (n + THREADS - 1) / THREADS;
    const int grid = (int)(blocks < FUSE_GRID ? blocks : FUSE_GRID);
    hipLaunchKernelGGL(fuse_fwd, dim3(grid), dim3(THREADS), 0, ecm_stream(stream), disp, var, prev, prev_var, prev_age, prev_source,
                       fused, fused_var, age, n, gate, process_noise, coast != 0);
    return ECM_LAUNCH_RESULT();
}
