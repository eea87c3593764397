// a8 + a9: disparity heads.  soft-argmin over D' for the three heads (cmfsm.py:703-706, 725-728,
// 748-753; disparityregression 111-123) and NN-upsample + 9-neighbour weighted sum
// (cmfsm.py:709-723, 730-744, 755-769).  All HBM/L2-bound, one thread per pixel column / HR pixel.
// The logits of a column are formed by column_sweep alone; the nine neighbours (c,l,r,t,b,lt,rt,lb,rb: cmfsm.py:551,585-593)
// are Nbr<0> of ecm_nbr.h, the table of the weight generators and of head_stats.hip / head_mode.hip.
#include "common.h"
#include "ecm_nbr.h"

namespace {

// ---- soft-argmin, heads fused: logits_k = c_0 + ... + c_k ----------------------------------
// One sweep of an LR column in the order of d: f(d, v), v[k] the logit of head k.  THE ONLY PLACE THIS HEAD'S LOGITS ARE FORMED
// in this file; every pass of softargmin_fwd and softargmin_bwd is one such sweep (a later pass re-reads from L2).
template <int NH, class F>
__device__ __forceinline__ void column_sweep(const float* __restrict__ base, long long hs, int D, int hw, F&& f) {
    for (int d = 0; d < D; ++d) {
        float acc = 0.f, v[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            acc += base[(size_t)k * hs + (size_t)d * hw];
            v[k] = acc;
        }
        f(d, v);
    }
}

// The column softmax both kernels start with: pass 1 the maxima (torch's softmax: exp(x - max) / sum), pass 2
// s = sum exp(logit - m) and t = sum exp(logit - m) d.
template <int NH>
__device__ __forceinline__ void column_softmax(const float* __restrict__ base, long long hs, int D, int hw, float (&m)[NH],
                                               float (&s)[NH], float (&t)[NH]) {
#pragma unroll
    for (int k = 0; k < NH; ++k) { m[k] = -INFINITY; s[k] = 0.f; t[k] = 0.f; }
    column_sweep<NH>(base, hs, D, hw, [&](int, const float (&v)[NH]) {
#pragma unroll
        for (int k = 0; k < NH; ++k) m[k] = fmaxf(m[k], v[k]);
    });
    column_sweep<NH>(base, hs, D, hw, [&](int d, const float (&v)[NH]) {
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            const float e = expf(v[k] - m[k]);
            s[k] += e;
            t[k] += e * (float)d;
        }
    });
}

// LSE: also lse[k,b,p] = m + ln s, the normaliser of head k's column, for aggregate9_stats_fwd
template <int NH, bool LSE = false>
__global__ __launch_bounds__(256) void softargmin_fwd(const float* __restrict__ c0, long long hs,
                                                      float* __restrict__ disp, float* __restrict__ lse, int B, int D,
                                                      int hw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // b*hw + p
    if (i >= (long long)B * hw) return;
    const int b = (int)(i / hw), p = (int)(i - (long long)b * hw);
    float m[NH], s[NH], t[NH];
    column_softmax<NH>(c0 + (size_t)b * D * hw + p, hs, D, hw, m, s, t);
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        disp[(size_t)k * B * hw + i] = t[k] / s[k];
        if constexpr (LSE) lse[(size_t)k * B * hw + i] = m[k] + logf(s[k]);
    }
}

// d disp_k / d logit_k[d] = p_k[d] (d - disp_k);  g c_j = sum_{k>=j} g logit_k
template <int NH>
__global__ __launch_bounds__(256) void softargmin_bwd(const float* __restrict__ c0, long long hs,
                                                      const float* __restrict__ gdisp, float* __restrict__ gc0,
                                                      int B, int D, int hw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * hw) return;
    const int b = (int)(i / hw), p = (int)(i - (long long)b * hw);
    const size_t off = (size_t)b * D * hw + p;
    float m[NH], s[NH], t[NH], g[NH];
    column_softmax<NH>(c0 + off, hs, D, hw, m, s, t);
    float inv[NH], dk[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) { inv[k] = 1.f / s[k]; dk[k] = t[k] * inv[k]; g[k] = gdisp[(size_t)k * B * hw + i]; }
    column_sweep<NH>(c0 + off, hs, D, hw, [&](int d, const float (&v)[NH]) {
        float gl[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) gl[k] = expf(v[k] - m[k]) * inv[k] * ((float)d - dk[k]) * g[k];
        float run = 0.f;
#pragma unroll
        for (int k = NH - 1; k >= 0; --k) {
            run += gl[k];
            gc0[off + (size_t)k * hs + (size_t)d * hw] = run;
        }
    });
}

__global__ __launch_bounds__(256) void dispreg_fwd(const float* __restrict__ x, float* __restrict__ out, int B, int D,
                                                   int hw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * hw) return;
    const int b = (int)(i / hw), p = (int)(i - (long long)b * hw);
    const float* base = x + (size_t)b * D * hw + p;
    float t = 0.f;
    for (int d = 0; d < D; ++d) t += base[(size_t)d * hw] * (float)d;
    out[i] = t;
}

// ---- 9-neighbour aggregation ----------------------------------------------------------------
// One thread per HR pixel; consecutive threads walk X so w9/out accesses are coalesced and the 3x3
// LR patch reads are broadcast within a cell (L1/L2 hits: d is 138 KB per head).
template <int NH>
__global__ __launch_bounds__(256) void aggregate9_fwd(const float* __restrict__ d, const float* __restrict__ w9,
                                                      float* __restrict__ out, int B, int h, int w, int s) {
    const int H = h * s, W = w * s;
    const long long HW = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;    // b*HW + Y*W + X
    if (i >= B * HW) return;
    const int b = (int)(i / HW);
    const int r = (int)(i - b * HW);
    const int Y = r / W, X = r - Y * W;
    const int cy = Y / s, cx = X / s;
    float acc[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) acc[k] = 0.f;
    const float fs = (float)s;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const int yy = cy + Nbr<0>::dy(n), xx = cx + Nbr<0>::dx(n);
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        const float wn = w9[((size_t)b * 9 + n) * HW + r];
#pragma unroll
        for (int k = 0; k < NH; ++k)
            acc[k] += (fs * d[((size_t)k * B + b) * h * w + (size_t)yy * w + xx]) * wn;
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) out[((size_t)k * B + b) * HW + r] = acc[k];
}

// gw9[b,n,Y,X] = sum_k gout[k,b,Y,X] * s * d[k,b,cell+n]   (0 where the neighbour is outside)
template <int NH>
__global__ __launch_bounds__(256) void aggregate9_bwd_w(const float* __restrict__ d, const float* __restrict__ gout,
                                                        float* __restrict__ gw9, int B, int h, int w, int s) {
    const int H = h * s, W = w * s;
    const long long HW = (long long)H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * HW) return;
    const int b = (int)(i / HW);
    const int r = (int)(i - b * HW);
    const int Y = r / W, X = r - Y * W;
    const int cy = Y / s, cx = X / s;
    float g[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) g[k] = gout[((size_t)k * B + b) * HW + r] * (float)s;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const int yy = cy + Nbr<0>::dy(n), xx = cx + Nbr<0>::dx(n);
        float v = 0.f;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
#pragma unroll
            for (int k = 0; k < NH; ++k) v += g[k] * d[((size_t)k * B + b) * h * w + (size_t)yy * w + xx];
        }
        gw9[((size_t)b * 9 + n) * HW + r] = v;
    }
}

// gd[k,b,cell] = s * sum_n sum_{pixels p of cell-n} w9[b,n,p] * gout[k,b,p]   (gather form, deterministic).
// One wave per (b, LR cell): lanes cover the 9 source cells' pixels.
template <int NH>
__global__ __launch_bounds__(256) void aggregate9_bwd_d(const float* __restrict__ w9, const float* __restrict__ gout,
                                                        float* __restrict__ gd, int B, int h, int w, int s) {
    const int H = h * s, W = w * s;
    const long long HW = (long long)H * W;
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // b*h*w + cy*w + cx
    if (cell >= (long long)B * h * w) return;      // wave-uniform
    const int b = (int)(cell / (h * w));
    const int c = (int)(cell - (long long)b * h * w);
    const int cy = c / w, cx = c - cy * w;
    float acc[NH];
#pragma unroll
    for (int k = 0; k < NH; ++k) acc[k] = 0.f;
    const int ss = s * s;
    for (int j = lane; j < 9 * ss; j += 64) {
        const int n = j / ss, q = j - n * ss;
        const int sy = cy - Nbr<0>::dy(n), sx = cx - Nbr<0>::dx(n);  // the HR cell whose plane-n weight points at (cy,cx)
        if (sy < 0 || sy >= h || sx < 0 || sx >= w) continue;
        const int Y = sy * s + q / s, X = sx * s + q % s;
        const size_t r = (size_t)Y * W + X;
        const float wn = w9[((size_t)b * 9 + n) * HW + r];
#pragma unroll
        for (int k = 0; k < NH; ++k) acc[k] += wn * gout[((size_t)k * B + b) * HW + r];
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const float v = wave_sum(acc[k]);
        if (lane == 0) gd[((size_t)k * B + b) * h * w + c] = v * (float)s;
    }
}

}  // namespace

// the plain head (lse == nullptr) and the one that also stores the normaliser: one grid
static int launch_softargmin_fwd(const float* c0, long long head_stride, float* disp, float* lse, int nheads, int B, int D,
                                 int hw, void* stream) {
    const long long n = (long long)B * hw;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return ecm_dispatch_heads(nheads, [&](auto nh) {
        constexpr int NH = decltype(nh)::value;
        const auto kernel = lse ? softargmin_fwd<NH, true> : softargmin_fwd<NH, false>;
        hipLaunchKernelGGL(kernel, grid, block, 0, ecm_stream(stream), c0, head_stride, disp, lse, B, D, hw);
        return ECM_LAUNCH_RESULT();
    });
}

extern "C" int ecm_softargmin_heads_fwd(const float* c0, long long head_stride, float* disp, int nheads, int B, int D,
                                        int hw, void* stream) {
    ECM_CHECK_ARG(c0 && disp && B > 0 && D > 0 && hw > 0);
    ECM_CHECK_HEADS(head_stride, nheads);
    return launch_softargmin_fwd(c0, head_stride, disp, nullptr, nheads, B, D, hw, stream);
}

extern "C" int ecm_softargmin_heads_lse_fwd(const float* c0, long long head_stride, float* disp, float* lse, int nheads,
                                            int B, int D, int hw, void* stream) {
    ECM_CHECK_ARG(c0 && disp && lse && B > 0 && D > 0 && hw > 0);
    ECM_CHECK_HEADS(head_stride, nheads);
    return launch_softargmin_fwd(c0, head_stride, disp, lse, nheads, B, D, hw, stream);
}

extern "C" int ecm_softargmin_heads_bwd(const float* c0, long long head_stride, const float* gdisp, float* gc0,
                                        int nheads, int B, int D, int hw, void* stream) {
    ECM_CHECK_ARG(c0 && gdisp && gc0 && B > 0 && D > 0 && hw > 0);
    ECM_CHECK_HEADS(head_stride, nheads);
    const long long n = (long long)B * hw;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return ecm_dispatch_heads(nheads, [&](auto nh) {
        hipLaunchKernelGGL(softargmin_bwd<decltype(nh)::value>, grid, block, 0, ecm_stream(stream), c0, head_stride, gdisp, gc0,
                           B, D, hw);
        return ECM_LAUNCH_RESULT();
    });
}

extern "C" int ecm_disparity_regression_fwd(const float* x, float* out, int B, int D, int hw, void* stream) {
    ECM_CHECK_ARG(x && out && B > 0 && D > 0 && hw > 0);
    const long long n = (long long)B * hw;
    hipLaunchKernelGGL(dispreg_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ecm_stream(stream), x, out, B, D,
                       hw);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_aggregate9_fwd(const float* d, const float* w9, float* out, int nheads, int B, int h, int w, int s,
                                  void* stream) {
    ECM_CHECK_ARG(d && w9 && out && B > 0 && h > 0 && w > 0 && s > 0);
    if (nheads < 1 || nheads > 3) return ECM_EUNSUP;
    const long long n = (long long)B * h * s * w * s;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return ecm_dispatch_heads(nheads, [&](auto nh) {
        hipLaunchKernelGGL(aggregate9_fwd<decltype(nh)::value>, grid, block, 0, ecm_stream(stream), d, w9, out, B, h, w, s);
        return ECM_LAUNCH_RESULT();
    });
}

extern "C" int ecm_aggregate9_bwd(const float* d, const float* w9, const float* gout, float* gd, float* gw9,
                                  int nheads, int B, int h, int w, int s, void* stream) {
    ECM_CHECK_ARG(d && w9 && gout && gd && gw9 && B > 0 && h > 0 && w > 0 && s > 0);
    if (nheads < 1 || nheads > 3) return ECM_EUNSUP;
    const long long n = (long long)B * h * s * w * s;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const long long cells = (long long)B * h * w;
    dim3 grid2((unsigned)((cells + 3) / 4));
    return ecm_dispatch_heads(nheads, [&](auto nh) {
        hipLaunchKernelGGL(aggregate9_bwd_w<decltype(nh)::value>, grid, block, 0, ecm_stream(stream), d, gout, gw9, B, h, w, s);
        hipLaunchKernelGGL(aggregate9_bwd_d<decltype(nh)::value>, grid2, block, 0, ecm_stream(stream), w9, gout, gd, B, h, w, s);
        return ECM_LAUNCH_RESULT();
    });
}
