// Image-space post-filters of a disparity map (include/ecm_hip.h has the definitions): the masked lower
// median over a (2r+1)^2 window, r = 1, 2, 3, and the joint bilateral filter guided by C = 1..4 image planes, r = 1..R_MAX.
// Both are LDS-tiled stencils, one launch each.  A workgroup of 256 threads owns a tile of TW x TH pixels at a time -- a wave is
// 64 consecutive x of one row and takes the rows wave, wave + 4 -- and walks tiles GRID apart:
//   stage    the tile plus a halo of r, row by row (a wave per row, lanes along x: coalesced), into LDS.  A sample that is not
//            usable -- outside the image, d not finite, valid == 0 -- is staged as NaN, so one compare (v == v) tells;
//   compute  median: the window into registers, the excluded samples replaced by -inf and +inf in turn, a sorting network of
//            compile-time comparators of which only rank (n-1)/2 is kept;  bilateral: a run-time loop over the window with the
//            centre's guide values in registers and the spatial exponents of one window row in LDS;
//   store    two planes, predicated on x < W.
// No atomics, no inline assembly, no private segment: every register array is indexed by compile-time constants only.
#include "disp_geom.h"
#include <utility>

namespace {

constexpr int THREADS = 256, WAVE = 64, NWAVE = THREADS / WAVE;
constexpr int TW = 64, TH = 8;                // the tile: a wave is one row of it, and takes TH / NWAVE rows
constexpr int GRID = 1024;                    // workgroups of a launch (four per CU); each walks tiles GRID apart
constexpr int MEDIAN_R_MAX = 3;               // 7 x 7: 49 values in registers
constexpr int R_MAX = 8;                      // bilateral: 17 x 17; LDS (1 + C)(TH + 2r)(TW + 2r) + 2r + 1 floats = 38,468 B at C = 4
constexpr int C_MAX = 4;

// ---- staging: the tile walk is disp_geom.h's --------------------------------------------------------------------------------------
// Stage rows y0-r .. y0+TH-1+r, columns x0-r .. x0+TW-1+r of the plane `src` (of image b) into dst [TH+2r][TW+2r].  MASKED: the
// disparity plane, NaN where the sample is not usable; else a guide plane, 0 outside the image (never looked at: d is NaN there).
template <bool MASKED>
__device__ __forceinline__ void stage_plane(float* dst, const float* __restrict__ src, const unsigned char* __restrict__ valid,
                                            int H, int W, int y0, int x0, int r) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int sw = TW + 2 * r, sh = TH + 2 * r;
    for (int ly = wave; ly < sh; ly += NWAVE) {
        const int y = y0 - r + ly;
        const bool yin = y >= 0 && y < H;                                  // wave-uniform
        for (int lx = lane; lx < sw; lx += WAVE) {
            const int x = x0 - r + lx;
            float v = MASKED ? __builtin_nanf("") : 0.f;
            if (yin && x >= 0 && x < W) {
                const size_t at = (size_t)y * W + x;
                v = MASKED ? ecm_disp_or_nan(src, valid, at) : src[at];
            }
            dst[ly * sw + lx] = v;
        }
    }
}

// ---- the median: a sorting network of compile-time comparators ---------------------------------------------------------------
// Batcher's odd-even merge sort of P = 64 wires, of which the comparators that touch a wire >= N are dropped: with +inf on the
// wires N..P-1 no comparator ever moves them (each puts the smaller value on the lower wire), so the first N wires are sorted by
// the comparators among themselves.  Only one output is read, so the compiler removes every comparator it does not depend on.
constexpr int NET_P = 64, NET_MAX = 543;       // comparators of the full 64-wire network
struct Net {
    int n;
    unsigned char lo[NET_MAX], hi[NET_MAX];
};
template <int N>
constexpr Net batcher() {
    Net net{};
    for (int p = 1; p < NET_P; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < NET_P; j += 2 * k)
                for (int i = 0; i < k && i + j + k < NET_P; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < N) {
                        net.lo[net.n] = (unsigned char)(i + j);
                        net.hi[net.n] = (unsigned char)(i + j + k);
                        ++net.n;
                    }
    return net;
}

template <int N>
struct Sorter {
    static constexpr Net net = batcher<N>();
    template <size_t... I>
    static __device__ __forceinline__ void run(float (&v)[N], std::index_sequence<I...>) {
        const int done[] = {(exchange(v[net.lo[I]], v[net.hi[I]]), 0)...};
        (void)done;
    }
    static __device__ __forceinline__ void exchange(float& a, float& b) {
        const float lo = fminf(a, b), hi = fmaxf(a, b);
        a = lo;
        b = hi;
    }
    static __device__ __forceinline__ void sort(float (&v)[N]) { run(v, std::make_index_sequence<net.n>{}); }
};

template <int R>
__global__ __launch_bounds__(THREADS) void disp_median_fwd(const float* __restrict__ d, const unsigned char* __restrict__ valid,
                                                           float* __restrict__ out, int B, int H, int W) {
    constexpr int K = 2 * R + 1, N = K * K, SW = TW + 2 * R, SH = TH + 2 * R;
    __shared__ float D[SH * SW];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const Tiles2D t = ecm_tiles_of<TW, TH>(B, H, W);
    const size_t image = (size_t)H * W, plane = (size_t)B * image;
    const float inf = __builtin_inff();

    for (long long tile = blockIdx.x; tile < t.n; tile += gridDim.x) {
        const int b = (int)(tile / ((long long)t.tx * t.ty));
        const int rest = (int)(tile - (long long)b * t.tx * t.ty);
        const int y0 = (rest / t.tx) * TH, x0 = (rest % t.tx) * TW;
        stage_plane<true>(D, d + b * image, valid ? valid + b * image : nullptr, H, W, y0, x0, R);
        __syncthreads();
#pragma unroll 1
        for (int ty = wave; ty < TH; ty += NWAVE) {
            const int y = y0 + ty, x = x0 + lane;
            if (y >= H) break;                                              // wave-uniform
            // the window, the excluded samples as -inf, +inf, -inf, ...: ceil(e/2) below and floor(e/2) above the m usable ones,
            // so that rank (N-1)/2 of the N is rank floor((m-1)/2) of the usable (DESIGN.md section 18 has the proof)
            float v[N];
            int m = 0;
            bool up = false;
#pragma unroll
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const float s = D[(ty + dy) * SW + lane + dx];
                    const bool ok = s == s;
                    v[dy * K + dx] = ok ? s : (up ? inf : -inf);
                    up = up != !ok;
                    m += ok ? 1 : 0;
                }
            Sorter<N>::sort(v);
            const float med = v[(N - 1) / 2];                              // finite iff m > 0
            if (x < W) {
                const size_t at = b * image + (size_t)y * W + x;
                out[at] = m > 0 ? med : 0.f;
                out[plane + at] = (float)m;
            }
        }
        __syncthreads();                                                    // the next tile overwrites D
    }
}

// ---- the joint bilateral filter -----------------------------------------------------------------------------------------------
// w(q) = exp2(ks (dx^2 + dy^2) + kc sum_c (g_c[p] - g_c[q])^2), ks = -log2(e) / (2 sigma_space^2), kc likewise of sigma_color.
template <int C>
__global__ __launch_bounds__(THREADS) void disp_bilateral_fwd(const float* __restrict__ d, const unsigned char* __restrict__ valid,
                                                              const float* __restrict__ guide, float* __restrict__ out, int B, int H,
                                                              int W, int r, float ks, float kc) {
    // LDS: D [SH][SW] the disparity, NaN where not usable; G [C][SH][SW] the guide; S [2r+1] = ks (i - r)^2, the spatial exponent
    // of an offset along one axis
    extern __shared__ float lds[];
    const int SW = TW + 2 * r, SH = TH + 2 * r, K = 2 * r + 1;
    float* D = lds;
    float* G = lds + SH * SW;
    float* S = lds + (1 + C) * SH * SW;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const Tiles2D t = ecm_tiles_of<TW, TH>(B, H, W);
    const size_t image = (size_t)H * W, plane = (size_t)B * image;

    if ((int)threadIdx.x < K) S[threadIdx.x] = ks * (float)(((int)threadIdx.x - r) * ((int)threadIdx.x - r));
    for (long long tile = blockIdx.x; tile < t.n; tile += gridDim.x) {
        const int b = (int)(tile / ((long long)t.tx * t.ty));
        const int rest = (int)(tile - (long long)b * t.tx * t.ty);
        const int y0 = (rest / t.tx) * TH, x0 = (rest % t.tx) * TW;
        stage_plane<true>(D, d + b * image, valid ? valid + b * image : nullptr, H, W, y0, x0, r);
#pragma unroll
        for (int c = 0; c < C; ++c) stage_plane<false>(G + c * SH * SW, guide + ((size_t)b * C + c) * image, nullptr, H, W, y0, x0, r);
        __syncthreads();
#pragma unroll 1
        for (int ty = wave; ty < TH; ty += NWAVE) {
            const int y = y0 + ty, x = x0 + lane;
            if (y >= H) break;                                              // wave-uniform
            float gp[C];
#pragma unroll
            for (int c = 0; c < C; ++c) gp[c] = G[c * SH * SW + (ty + r) * SW + lane + r];
            float sw = 0.f, swd = 0.f;
            for (int dy = 0; dy < K; ++dy) {
                const float sy = S[dy];
                const int row = (ty + dy) * SW + lane;
                for (int dx = 0; dx < K; ++dx) {
                    const float dq = D[row + dx];
                    float dist = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float diff = gp[c] - G[c * SH * SW + row + dx];
                        dist = fmaf(diff, diff, dist);
                    }
                    const float e = fmaf(kc, dist, sy + S[dx]);
                    const bool ok = dq == dq && e == e;                     // usable, and no NaN from a non-finite guide value
                    const float w = ok ? __builtin_amdgcn_exp2f(e) : 0.f;
                    sw += w;
                    swd = fmaf(w, ok ? dq : 0.f, swd);
                }
            }
            if (x < W) {
                const size_t at = b * image + (size_t)y * W + x;
                out[at] = sw > 0.f ? swd / sw : 0.f;
                out[plane + at] = sw;
            }
        }
        __syncthreads();                                                    // the next tile overwrites D and G
    }
}

inline bool sizes_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0; }
inline bool too_large(int B, int H, int W) { return (long long)B * H * W > INT_MAX; }
inline int grid_of(int B, int H, int W) {
    const long long n = ecm_tiles_of<TW, TH>(B, H, W).n;
    return (int)(n < GRID ? n : GRID);
}

}  // namespace

extern "C" int ecm_disp_filter_max_radius(int kind) {
    return kind == ECM_DISP_FILTER_MEDIAN ? MEDIAN_R_MAX : kind == ECM_DISP_FILTER_BILATERAL ? R_MAX : ECM_EINVAL;
}

extern "C" int ecm_disp_median_fwd(const float* d, const unsigned char* valid, float* out, int B, int H, int W, int radius,
                                   void* stream) {
    ECM_CHECK_ARG(d && out && sizes_ok(B, H, W) && radius >= 1 && radius <= MEDIAN_R_MAX);
    if (too_large(B, H, W)) return ECM_EUNSUP;
    const dim3 grid(grid_of(B, H, W)), block(THREADS);
    hipStream_t s = ecm_stream(stream);
    if (radius == 1) hipLaunchKernelGGL(disp_median_fwd<1>, grid, block, 0, s, d, valid, out, B, H, W);
    else if (radius == 2) hipLaunchKernelGGL(disp_median_fwd<2>, grid, block, 0, s, d, valid, out, B, H, W);
    else hipLaunchKernelGGL(disp_median_fwd<3>, grid, block, 0, s, d, valid, out, B, H, W);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_disp_bilateral_fwd(const float* d, const unsigned char* valid, const float* guide, float* out, int B, int C,
                                      int H, int W, int radius, float sigma_space, float sigma_color, void* stream) {
    const float inf = __builtin_inff();
    ECM_CHECK_ARG(d && guide && out && sizes_ok(B, H, W) && C >= 1 && C <= C_MAX && radius >= 1 && radius <= R_MAX &&
                  sigma_space > 0.f && sigma_space < inf && sigma_color > 0.f && sigma_color < inf);
    if (too_large(B, H, W)) return ECM_EUNSUP;
    const float log2e = 1.44269504088896340736f;
    const float ks = -log2e / (2.f * sigma_space * sigma_space), kc = -log2e / (2.f * sigma_color * sigma_color);
    ECM_CHECK_ARG(ks > -inf && kc > -inf);                                   // a sigma whose square underflows
    const dim3 grid(grid_of(B, H, W)), block(THREADS);
    const size_t lds = ((size_t)(1 + C) * (TH + 2 * radius) * (TW + 2 * radius) + 2 * radius + 1) * sizeof(float);
    hipStream_t s = ecm_stream(stream);
    switch (C) {
        case 1: hipLaunchKernelGGL(disp_bilateral_fwd<1>, grid, block, lds, s, d, valid, guide, out, B, H, W, radius, ks, kc); break;
        case 2: hipLaunchKernelGGL(disp_bilateral_fwd<2>, grid, block, lds, s, d, valid, guide, out, B, H, W, radius, ks, kc); break;
        case 3: hipLaunchKernelGGL(disp_bilateral_fwd<3>, grid, block, lds, s, d, valid, guide, out, B, H, W, radius, ks, kc); break;
        default: hipLaunchKernelGGL(disp_bilateral_fwd<4>, grid, block, lds, s, d, valid, guide, out, B, H, W, radius, ks, kc); break;
    }
    return ECM_LAUNCH_RESULT();
}
