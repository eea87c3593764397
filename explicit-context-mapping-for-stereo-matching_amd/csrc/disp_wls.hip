// The WLS disparity smoother (include/ecm_hip.h has the definitions): the confidence-weighted fast global
// smoother of Min et al. 2014, OpenCV's DisparityWLSFilter.  N = conf * d and D = conf go through T rounds of "every row, then
// every column" of the tridiagonal solve (I + lambda_t A) u = f, A the Laplacian of the guide's link weights; smoothed = N / D.
// 2T launches of one kernel body on the one stream, a horizontal and a vertical pass per round:
//   lines    a workgroup of 256 threads owns LINES lines (rows in the horizontal pass, columns in the vertical one) and walks them
//            in chunks of CHUNK positions.  ONE LANE OWNS ONE LINE and runs the plain sequential Thomas recurrence in natural
//            order, which keeps the rounding comparable with the restatement in tests/test_disp_wls_cpu.py;
//   stage    per chunk the whole workgroup loads the tile coalesced (a thread's consecutive lanes are consecutive x in both
//            passes), computes what is not on the dependent chain -- the usable test and conf * d in the first pass, the link
//            weight to the next position with its sqrt and exp, c_i = -lambda_t w_i -- and puts it into LDS, transposed for the
//            horizontal pass (stride CHUNK + 1: the lanes of the sweep read distinct banks);
//   sweep    lanes 0..LINES-1 of wave 0: forward den = b - a c', one division, three multiplies and three FMAs per position
//            (a_i is the c_{i-1} the lane carries, b_i = 1 - a_i - c_i two subtractions off the chain), results back into the
//            tile; the next chunk's global loads were issued before the sweep and are waited for after it;
//   store    the whole workgroup writes c' (scratch) and N', D' (`out`) coalesced; after the last chunk the same walk in reverse
//            reloads them and the lanes run u_i = f'_i - c'_i u_{i+1}, one FMA per position and plane.
// N and D go through the same instructions with the same coefficients, so a constant power-of-two plane comes back bit for bit
// and a region that cut links separate from every confident pixel has D == 0 exactly.  Written with explicit fmaf so that no
// contraction can treat the two planes differently.  No atomics, no workgroup waits for another, no private segment.
#include "disp_geom.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE = 1024;                    // positions of a staged tile: LINES * CHUNK in both passes
constexpr int PER = TILE / THREADS;           // tile elements per thread
constexpr int LINES = 16, CHUNK = 64;         // the horizontal pass: rows per workgroup, columns per chunk
constexpr int VLINES = 32, VCHUNK = 32;       // the vertical pass: columns per workgroup, rows per chunk
constexpr int C_MAX = 4, T_MAX = 8;
constexpr int PAD = 1;                        // the horizontal tile's row stride is CHUNK + PAD

template <bool VERT>
struct Geo {
    static constexpr int NL = VERT ? VLINES : LINES, NC = VERT ? VCHUNK : CHUNK;
    static constexpr int TX = VERT ? NL : NC;                                   // the tile's extent along x
    static constexpr int WORDS = VERT ? NC * NL : NL * (NC + PAD);
    __device__ static __forceinline__ int at(int line, int pos) { return VERT ? pos * NL + line : line * (NC + PAD) + pos; }
};

struct Raw {                                  // what a thread has in flight for one tile element
    float n, d;                               // d and conf in the first pass, N and D after it
    float g[C_MAX], gq[C_MAX];                // the guide here and at the next position of the line
};

// One pass over the lines of one direction.  in_n / in_d: d and conf (conf may be null) where `first`, else the N and D planes of
// `out`; out_n / out_d the planes of `out`; cp the c' plane.  No __restrict__ on the planes that are both written and read.
template <bool VERT>
__global__ __launch_bounds__(THREADS) void wls_pass(const float* in_n, const float* in_d, const float* __restrict__ guide,
                                                    float* out_n, float* out_d, float* cp, int B, int C, int H, int W,
                                                    float lam_t, float sigma, int first, int last) {
    using G = Geo<VERT>;
    __shared__ float TC[G::WORDS], TN[G::WORDS], TD[G::WORDS];
    const int nlines = VERT ? W : H, n = VERT ? H : W;                          // lines of an image, positions of a line
    const int groups = (nlines + G::NL - 1) / G::NL, nchunks = (n + G::NC - 1) / G::NC;
    const int b = blockIdx.x / groups, line0 = (blockIdx.x - b * groups) * G::NL;
    const size_t image = (size_t)H * W, base = (size_t)b * image;
    const float* gi = guide + (size_t)b * C * image;
    const size_t step = VERT ? (size_t)W : 1;                                   // to the next position of a line
    const int tid = threadIdx.x;

    int tl[PER], tp[PER];                     // a thread's tile elements: line and position within the tile
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int e = tid + k * THREADS, ex = e % G::TX, ey = e / G::TX;
        tl[k] = VERT ? ex : ey;
        tp[k] = VERT ? ey : ex;
    }
    auto pixel = [&](int line, int pos) { return VERT ? (size_t)pos * W + line : (size_t)line * W + pos; };

    Raw raw[PER];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int line = line0 + tl[k], pos = chunk * G::NC + tp[k];
            raw[k].n = raw[k].d = 0.f;
#pragma unroll
            for (int c = 0; c < C_MAX; ++c) raw[k].g[c] = raw[k].gq[c] = 0.f;
            if (line < nlines && pos < n) {
                const size_t p = pixel(line, pos);
                raw[k].n = in_n[base + p];
                raw[k].d = in_d ? in_d[base + p] : 1.f;
                if (pos + 1 < n) {
#pragma unroll
                    for (int c = 0; c < C_MAX; ++c)
                        if (c < C) {
                            raw[k].g[c] = gi[c * image + p];
                            raw[k].gq[c] = gi[c * image + p + step];
                        }
                }
            }
        }
    };

    // ---- forward -------------------------------------------------------------------------------------------------------------
    float c_prev = 0.f, cp_prev = 0.f, n_prev = 0.f, d_prev = 0.f;               // c_{i-1}, c'_{i-1}, N'_{i-1}, D'_{i-1}
    fetch(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int pos = chunk * G::NC + tp[k];
            float fn = raw[k].n, fd = raw[k].d;
            if (first) {                                                        // usable: both finite, conf >= 0; else both 0
                const bool ok = ecm_finite(fn) && ecm_finite(fd) && fd >= 0.f;
                fd = ok ? fd : 0.f;
                fn = ok ? fd * fn : 0.f;
            }
            float c = 0.f;
            if (pos + 1 < n) {
                float s = 0.f;
#pragma unroll
                for (int ch = 0; ch < C_MAX; ++ch)
                    if (ch < C) {
                        const float t = raw[k].g[ch] - raw[k].gq[ch];
                        s = __builtin_fmaf(t, t, s);
                    }
                float w = expf(-sqrtf(s) / sigma);
                w = w == w ? w : 0.f;                                           // a NaN weight cuts the link
                c = -lam_t * w;
            }
            const int i = G::at(tl[k], tp[k]);
            TC[i] = c;
            TN[i] = fn;
            TD[i] = fd;
        }
        __syncthreads();
        if (chunk + 1 < nchunks) fetch(chunk + 1);                              // in flight during the sweep
        const int len = min(G::NC, n - chunk * G::NC);
        if (tid < G::NL && line0 + tid < nlines) {
#pragma unroll 4
            for (int j = 0; j < len; ++j) {
                const int i = G::at(tid, j);
                const float c = TC[i], a = c_prev;
                const float bb = (1.f - a) - c;
                const float den = __builtin_fmaf(-a, cp_prev, bb);
                const float inv = 1.f / den;
                cp_prev = c * inv;
                n_prev = __builtin_fmaf(-a, n_prev, TN[i]) * inv;
                d_prev = __builtin_fmaf(-a, d_prev, TD[i]) * inv;
                c_prev = c;
                TC[i] = cp_prev;
                TN[i] = n_prev;
                TD[i] = d_prev;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int line = line0 + tl[k], pos = chunk * G::NC + tp[k];
            if (line < nlines && pos < n) {
                const size_t p = base + pixel(line, pos);
                const int i = G::at(tl[k], tp[k]);
                cp[p] = TC[i];
                out_n[p] = TN[i];
                out_d[p] = TD[i];
            }
        }
        __syncthreads();                                                        // the next chunk overwrites the tiles
    }

    // ---- backward: every thread reloads what it stored itself ----------------------------------------------------------------
    float un = 0.f, ud = 0.f;                                                   // u_{i+1}; c'_{n-1} is 0
    float rc[PER], rn[PER], rd[PER];
    auto reload = [&](int chunk) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int line = line0 + tl[k], pos = chunk * G::NC + tp[k];
            rc[k] = rn[k] = rd[k] = 0.f;
            if (line < nlines && pos < n) {
                const size_t p = base + pixel(line, pos);
                rc[k] = cp[p];
                rn[k] = out_n[p];
                rd[k] = out_d[p];
            }
        }
    };
    reload(nchunks - 1);
    for (int chunk = nchunks - 1; chunk >= 0; --chunk) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = G::at(tl[k], tp[k]);
            TC[i] = rc[k];
            TN[i] = rn[k];
            TD[i] = rd[k];
        }
        __syncthreads();
        if (chunk > 0) reload(chunk - 1);
        const int len = min(G::NC, n - chunk * G::NC);
        if (tid < G::NL && line0 + tid < nlines) {
#pragma unroll 4
            for (int j = len - 1; j >= 0; --j) {
                const int i = G::at(tid, j);
                const float c = TC[i];
                un = __builtin_fmaf(-c, un, TN[i]);
                ud = __builtin_fmaf(-c, ud, TD[i]);
                TN[i] = un;
                TD[i] = ud;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int line = line0 + tl[k], pos = chunk * G::NC + tp[k];
            if (line < nlines && pos < n) {
                const size_t p = base + pixel(line, pos);
                const int i = G::at(tl[k], tp[k]);
                const float vn = TN[i], vd = TD[i];
                out_n[p] = last ? (vd > 0.f ? vn / vd : 0.f) : vn;
                out_d[p] = vd;
            }
        }
        __syncthreads();
    }
}

inline bool positive(float v) { return v > 0.f && v < __builtin_inff(); }

}  // namespace

extern "C" long long ecm_disp_wls_scratch_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return ECM_EINVAL;
    if ((long long)B * H * W > INT_MAX) return 0;                                  // what ecm_disp_wls_fwd answers ECM_EUNSUP
    return (long long)B * H * W * (long long)sizeof(float);                     // the c' plane
}

extern "C" int ecm_disp_wls_fwd(const float* d, const float* conf, const float* guide, float* out, void* scratch, int B, int C,
                                int H, int W, float lam, float sigma_color, int iterations, void* stream) {
    ECM_CHECK_ARG(d && guide && out && scratch && B > 0 && H > 0 && W > 0 && C >= 1 && C <= C_MAX && positive(lam) &&
                  positive(sigma_color) && iterations >= 1 && iterations <= T_MAX);
    if ((long long)B * H * W > INT_MAX) return ECM_EUNSUP;
    const size_t plane = (size_t)B * H * W;
    float* on = out;
    float* od = out + plane;
    float* cp = static_cast<float*>(scratch);
    const int T = iterations;
    const double all = std::ldexp(1.0, 2 * T) - 1.0;                            // 4^T - 1
    const dim3 block(THREADS);
    const dim3 rows((unsigned)((long long)B * ((H + LINES - 1) / LINES))), cols((unsigned)((long long)B * ((W + VLINES - 1) / VLINES)));
    hipStream_t s = ecm_stream(stream);
    for (int t = 1; t <= T; ++t) {
        const float lam_t = (float)(1.5 * std::ldexp(1.0, 2 * (T - t)) / all * (double)lam);
        const int first = t == 1, last = t == T;
        hipLaunchKernelGGL(wls_pass<false>, rows, block, 0, s, first ? d : on, first ? conf : od, guide, on, od, cp, B, C, H, W,
                           lam_t, sigma_color, first, 0);
        hipLaunchKernelGGL(wls_pass<true>, cols, block, 0, s, on, od, guide, on, od, cp, B, C, H, W, lam_t, sigma_color, 0, last);
    }
    return ECM_LAUNCH_RESULT();
}
