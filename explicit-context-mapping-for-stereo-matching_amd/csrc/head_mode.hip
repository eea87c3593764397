// The modal disparity of the eight-neighbour head: per full-resolution pixel the highest level D* of the
// mixture p(d) = sum_n a_n p_n(d) of its valid neighbours' low-resolution distributions (section 15), the mass of p in the
// window |d - D*| <= r and p's mean inside that window.  The volume and trilinear heads' modal estimate is MODE 2 of their own
// kernels (variants.hip); this file is the LDS-staged mixture kernel that section 15 named as the follow-up of
// aggregate9_stats_fwd: a workgroup normalises the cell columns under its tile ONCE and its pixels mix from LDS, with no
// exponential of their own.  Which neighbours a pixel mixes and with what weights is ecm_mixture9 (ecm_nbr.h), shared with
// head_stats.hip; that kernel reads its columns from global memory, this one from LDS.
#include "common.h"
#include "ecm_nbr.h"

namespace {

constexpr int TX = 64, TY = 4;            // the tile of full-resolution pixels: a wave is 64 consecutive X, a workgroup four rows
constexpr int DC_MAX = 48;                // at most this many levels are staged at a time (D' = 48 at 576 x 960: one chunk)
constexpr int LDS_BUDGET = 64 * 1024;     // what a kernel may ask for without raising its limit

// cells under `n` pixels that start at a multiple of n, plus one cell of halo on each side
__host__ __device__ constexpr int span_cells(int n, int s) { return (n % s == 0 ? n / s : (n - 1) / s + 2) + 2; }

// LDS: P [NH][dc][ncol] the normalised columns of the current chunk of levels, then S [NH][ncol] the columns' normalisers,
// L [NH][ncol] their shifts (lse) and Kc [NH][ncol] the running compensation of the normalisers' sums.  A column is a cell of
// the tile's footprint plus halo, [row][x] with x fastest, so the lanes of a wave (consecutive X of one row) read consecutive
// columns with an s-fold broadcast.  Columns outside the image hold zeros and are given weight zero: the sweeps need no branch
// on validity.
template <int NH>
__global__ __launch_bounds__(256) void aggregate9_mode_fwd(const float* __restrict__ c0, long long hs,
                                                           const float* __restrict__ lse, const float* __restrict__ w9,
                                                           float* __restrict__ modal, int B, int D, int h, int w, int s, int r,
                                                           int dc, int ncol_max) {
    extern __shared__ float lds[];
    const int H = h * s, W = w * s, hw = h * w;
    const long long HW = (long long)H * W;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int X0 = blockIdx.x * TX, Y0 = blockIdx.y * TY;
    const int X1 = min(X0 + TX, W) - 1, Y1 = min(Y0 + TY, H) - 1;     // the tile's last pixel inside the image
    const int cx0 = X0 / s - 1, cy0 = Y0 / s - 1;                     // the first staged column (halo: may be -1)
    const int ncx = X1 / s - cx0 + 2, ncy = Y1 / s - cy0 + 2;
    const int ncol = ncx * ncy;                                       // <= ncol_max, what the host sized the arrays by
    float* P = lds;
    float* S = lds + (size_t)NH * dc * ncol_max;
    float* L = S + (size_t)NH * ncol_max;
    float* Kc = L + (size_t)NH * ncol_max;
    const float* base = c0 + (size_t)b * D * hw;

    // global cell of a staged column, -1 outside the image
    auto cell_of = [&](int col) {
        const int yy = cy0 + col / ncx, xx = cx0 + col % ncx;
        return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? yy * w + xx : -1;
    };
    for (int it = tid; it < NH * ncol; it += 256) {
        const int k = it / ncol, col = it - k * ncol, cell = cell_of(col);
        L[it] = cell >= 0 ? lse[((size_t)k * B + b) * hw + cell] : 0.f;
        S[it] = 0.f;
        Kc[it] = 0.f;
    }
    __syncthreads();
    // levels [d0, d0 + nd) into P: exp(logit - lse), times the column's 1 / sum once that is known (scaled)
    auto stage = [&](int d0, int nd, bool scaled) {
        for (int it = tid; it < nd * ncol; it += 256) {
            const int dd = it / ncol, col = it - dd * ncol, cell = cell_of(col);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                float e = 0.f;
                if (cell >= 0) {
                    acc += base[(size_t)k * hs + (size_t)(d0 + dd) * hw + cell];
                    e = expf(acc - L[k * ncol + col]);
                    if (scaled) e *= S[k * ncol + col];
                }
                P[((size_t)k * dc + dd) * ncol + col] = e;
            }
        }
    };
    // The exact normaliser (section 15: lse is one rounded float, the shift only): every column's sum over ALL levels, each
    // (head, column) by one thread in the order of d, as a compensated (Kahan) sum: a plain running sum of D' equal terms --
    // a flat column -- rounds the same way at every step and was 10 ulp off at D' = 55.  With one chunk that thread then
    // scales its column in place.
    const int nchunk = (D + dc - 1) / dc;
    for (int d0 = 0; d0 < D; d0 += dc) {
        const int nd = min(dc, D - d0);
        stage(d0, nd, false);
        __syncthreads();
        for (int it = tid; it < NH * ncol; it += 256) {
            const int k = it / ncol, col = it - k * ncol;
            float* p = P + (size_t)k * dc * ncol + col;
            float sum = S[it], comp = Kc[it];
            for (int dd = 0; dd < nd; ++dd) {
                const float y = p[(size_t)dd * ncol] - comp, t = sum + y;
                comp = (t - sum) - y;
                sum = t;
            }
            Kc[it] = comp;
            if (d0 + nd == D) {
                sum = cell_of(col) >= 0 ? 1.f / sum : 0.f;
                if (nchunk == 1)
                    for (int dd = 0; dd < nd; ++dd) p[(size_t)dd * ncol] *= sum;
            }
            S[it] = sum;
        }
        __syncthreads();
    }

    // this thread's pixel: the nine columns and the weights a_n = w9[n] / sum of the valid w9 (zero for a skipped neighbour)
    const int X = X0 + (tid & 63), Y = Y0 + (tid >> 6);
    const bool live = X < W && Y < H;
    const int Xc = live ? X : X0, Yc = live ? Y : Y0;
    const int pix = Yc * W + Xc;
    const int lc = (Yc / s - cy0) * ncx + (Xc / s - cx0);             // the centre's column: inside the halo ring
    float a[9];
    int off[9], cell[9];
    ecm_mixture9(w9 + (size_t)b * 9 * HW + pix, HW, Yc / s, Xc / s, h, w, a, cell);
#pragma unroll
    for (int n = 0; n < 9; ++n) off[n] = lc + Nbr<0>::dy(n) * ncx + Nbr<0>::dx(n);
    auto mix = [&](int k, int dd) {
        const float* p = P + ((size_t)k * dc + dd) * ncol;
        float v = 0.f;
#pragma unroll
        for (int n = 0; n < 9; ++n) v = fmaf(a[n], p[off[n]], v);
        return v;
    };

    // sweep 1: all levels, the first maximum (strict >); tot keeps a NaN that the comparison drops
    float best[NH], tot[NH];
    int dstar[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) { best[k] = -1.f; tot[k] = 0.f; dstar[k] = 0; }
    for (int d0 = 0; d0 < D; d0 += dc) {
        const int nd = min(dc, D - d0);
        if (nchunk > 1) { stage(d0, nd, true); __syncthreads(); }
        if (live) {
            for (int dd = 0; dd < nd; ++dd) {
#pragma unroll
                for (int k = 0; k < NH; ++k) {
                    const float v = mix(k, dd);
                    tot[k] += v;
                    if (v > best[k]) { best[k] = v; dstar[k] = d0 + dd; }
                }
            }
        }
        if (nchunk > 1) __syncthreads();
    }
    // sweep 2: the at most 2 r + 1 levels of the window about D*, centred on it
    float sw[NH], cw[NH], sm[NH];                                     // sw: compensated as the normalisers are
#pragma unroll
    for (int k = 0; k < NH; ++k) { sw[k] = 0.f; cw[k] = 0.f; sm[k] = 0.f; }
    for (int d0 = 0; d0 < D; d0 += dc) {
        const int nd = min(dc, D - d0);
        if (nchunk > 1) { stage(d0, nd, true); __syncthreads(); }
        if (live) {
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                const int lo = max(dstar[k] - r, d0), hi = min(dstar[k] + r, d0 + nd - 1);
                for (int d = lo; d <= hi; ++d) {
                    const float v = mix(k, d - d0);
                    const float y = v - cw[k], t = sw[k] + y;
                    cw[k] = (t - sw[k]) - y;
                    sw[k] = t;
                    sm[k] = fmaf(v, (float)(d - dstar[k]), sm[k]);
                }
            }
        }
        if (nchunk > 1) __syncthreads();
    }
    if (!live) return;
    const float fs = (float)s;
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const bool nan = tot[k] != tot[k];
        float* o = modal + (((size_t)k * 3) * B + b) * HW + pix;
        o[0] = nan ? tot[k] : fs * ((float)dstar[k] + sm[k] / sw[k]);
        o[(size_t)B * HW] = nan ? tot[k] : fminf(sw[k], 1.f);
        o[(size_t)2 * B * HW] = nan ? tot[k] : fs * (float)dstar[k];
    }
}

}  // namespace

extern "C" int ecm_aggregate9_mode_fwd(const float* c0, long long head_stride, const float* lse, const float* w9, float* modal,
                                       int nheads, int B, int D, int h, int w, int s, int radius, void* stream) {
    ECM_CHECK_ARG(c0 && lse && w9 && modal && B > 0 && D > 0 && h > 0 && w > 0 && s > 0 && radius >= 0 && radius % s == 0);
    ECM_CHECK_HEADS(head_stride, nheads);                            // nheads sizes the LDS below
    if (B > 65535) return ECM_EUNSUP;
    const int ncol = span_cells(TX, s) * span_cells(TY, s);
    // the levels that fit beside S, L and Kc; at s = 4: 54 columns, 48 levels x 3 heads = 31,104 B + 1,944 B
    const int dc = min(min(D, DC_MAX), (LDS_BUDGET / (int)sizeof(float) - 3 * nheads * ncol) / (nheads * ncol));
    if (dc < 1) return ECM_EUNSUP;        // cannot happen at TX x TY = 64 x 4 (s = 1: 396 columns, 10 levels); kept for other tiles
    const size_t lds = ((size_t)nheads * dc + 3 * (size_t)nheads) * ncol * sizeof(float);
    const int r = min(radius / s, D);
    dim3 grid((w * s + TX - 1) / TX, (h * s + TY - 1) / TY, B), block(256);
    return ecm_dispatch_heads(nheads, [&](auto nh) {
        hipLaunchKernelGGL(aggregate9_mode_fwd<decltype(nh)::value>, grid, block, lds, ecm_stream(stream), c0, head_stride, lse, w9,
                           modal, B, D, h, w, s, r, dc, ncol);
        return ECM_LAUNCH_RESULT();
    });
}
