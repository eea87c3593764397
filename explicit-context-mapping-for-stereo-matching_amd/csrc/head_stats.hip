// Per-pixel uncertainty of the eight-neighbour head: std, peak and entropy of each full-resolution
// pixel's mixture of its neighbours' low-resolution distributions.  The head itself is heads.hip (softargmin_fwd with LSE,
// aggregate9_fwd); this kernel reads the same classifier outputs, the same w9 and the normalisers softargmin_fwd stored.  Which
// neighbours a pixel mixes and with what weights is ecm_mixture9 (ecm_nbr.h), shared with head_mode.hip.
#include "common.h"
#include "ecm_nbr.h"

namespace {

// Statistics of the HR pixel's distribution: the mixture p(d) = sum_n a_n p_n(d) of the low-resolution
// softmaxes of the neighbours aggregate9_fwd does not skip, a_n = w9[n] / sum of the valid w9.  p_n(d) = exp(logit_n(d) - lse_n).
// The sweep over d: mean and centred second moment by the weighted Welford update (each term a product of non-negative
// factors, no difference of large sums), peak and entropy directly.  The s*s pixels of a cell read the same nine columns: a
// wave's load of one neighbour touches 64/s consecutive cells, one or two cache lines, and is served by L1/L2 (section 15).
template <int NH>
__global__ __launch_bounds__(256) void aggregate9_stats_fwd(const float* __restrict__ c0, long long hs,
                                                            const float* __restrict__ lse, const float* __restrict__ w9,
                                                            float* __restrict__ stats, int B, int D, int h, int w, int s) {
    const int H = h * s, W = w * s;
    const long long HW = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;    // b*HW + Y*W + X
    if (i >= B * HW) return;
    const int b = (int)(i / HW);
    const int r = (int)(i - b * HW);
    const int Y = r / W, X = r - Y * W;
    const int cy = Y / s, cx = X / s;
    const int hw = h * w;
    float a[9], ln[9][NH];
    int cell[9];
    ecm_mixture9(w9 + (size_t)b * 9 * HW + r, HW, cy, cx, h, w, a, cell);
#pragma unroll
    for (int n = 0; n < 9; ++n)
#pragma unroll
        for (int k = 0; k < NH; ++k) ln[n][k] = cell[n] >= 0 ? lse[((size_t)k * B + b) * hw + cell[n]] : 0.f;
    const float* base = c0 + (size_t)b * D * hw;
    // lse is one rounded float: at |lse| ~ 100 it is off by 4e-6, and so would every p_n be.  It serves as the shift that keeps
    // the exponentials in range; a first sweep sums them and folds the exact normaliser into the weight, an = a_n / sum.
    float an[9][NH];
#pragma unroll
    for (int n = 0; n < 9; ++n)
#pragma unroll
        for (int k = 0; k < NH; ++k) an[n][k] = 0.f;
    for (int d = 0; d < D; ++d) {
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            if (cell[n] < 0) continue;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                acc += base[(size_t)k * hs + (size_t)d * hw + cell[n]];
                an[n][k] += expf(acc - ln[n][k]);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < 9; ++n)
#pragma unroll
        for (int k = 0; k < NH; ++k) an[n][k] = a[n] / an[n][k];
    float S[NH], mu[NH], M2[NH], pk[NH], en[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) { S[k] = 0.f; mu[k] = 0.f; M2[k] = 0.f; pk[k] = 0.f; en[k] = 0.f; }
    for (int d = 0; d < D; ++d) {
        float p[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) p[k] = 0.f;
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            if (cell[n] < 0) continue;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                acc += base[(size_t)k * hs + (size_t)d * hw + cell[n]];
                p[k] = fmaf(an[n][k], expf(acc - ln[n][k]), p[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            const float Sn = S[k] + p[k];
            if (p[k] > 0.f) {                                            // 0 ln 0 = 0, and Sn > 0 below
                const float delta = (float)d - mu[k], f = p[k] / Sn;
                mu[k] = fmaf(f, delta, mu[k]);
                M2[k] = fmaf(S[k] * f, delta * delta, M2[k]);
                en[k] = fmaf(-p[k], logf(p[k]), en[k]);
            }
            S[k] = Sn;                                                   // a NaN p skips the branch and lands here
            pk[k] = fmaxf(pk[k], p[k]);
        }
    }
    const float fs = (float)s;
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const bool nan = S[k] != S[k];                                   // fmaxf and the branch above drop a NaN; S keeps it
        float* o = stats + (((size_t)k * 3) * B + b) * HW + r;
        o[0] = nan ? S[k] : fs * sqrtf(M2[k] / S[k]);
        o[(size_t)B * HW] = nan ? S[k] : fminf(pk[k], 1.f);
        o[(size_t)2 * B * HW] = nan ? S[k] : fmaxf(en[k], 0.f);
    }
}

}  // namespace

extern "C" int ecm_aggregate9_stats_fwd(const float* c0, long long head_stride, const float* lse, const float* w9,
                                        float* stats, int nheads, int B, int D, int h, int w, int s, void* stream) {
    ECM_CHECK_ARG(c0 && lse && w9 && stats && B > 0 && D > 0 && h > 0 && w > 0 && s > 0);
    ECM_CHECK_HEADS(head_stride, nheads);
    const long long n = (long long)B * h * s * w * s;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return ecm_dispatch_heads(nheads, [&](auto nh) {
        hipLaunchKernelGGL(aggregate9_stats_fwd<decltype(nh)::value>, grid, block, 0, ecm_stream(stream), c0, head_stride, lse, w9,
                           stats, B, D, h, w, s);
        return ECM_LAUNCH_RESULT();
    });
}
