// Eval leg of the harness, on the device:
//   * SceneFlow evaluation, test.py:69-94 -- prediction and ground truth cropped to [:crop_h, :crop_w] (540 x 960: the
//     loader pads frames to 576 rows), three masks over the ground truth d at column x
//         mask      = 0 <= d < maxdisp
//         mask_non  = mask and x - d >= 0          (the matching pixel lies inside the target image)
//         mask_true = 0 <  d < maxdisp and x - d >= 0
//     and the mean absolute error of `output3` under each.  The reference gathers o[mask] six times (a host sync each).
//   * KITTI submission image, test_kitti.py:163-168 -- output3 * 256 -> uint16 (C cast: truncation), un-pad
//     `pre[0, -h:, -w:]` (the loader pads at the TOP and LEFT, KITTI.py:99-108).  Integer output: bit-exact.
//   * KITTI validation, eval_kitti.py:84-103 -- output3 on the whole (top/left padded) frame, no crop, d > 0 masks
//         mask = 0 < d < maxdisp;   mask_non = mask_true = mask and x - d >= 0
//     the three masked mean errors and the 3-px / 5 % error rate of the batch, and the same eight columns per image.
// One streaming pass each; EPE sums go through per-workgroup partials and a fixed-order final sum in double.
#include "common.h"
#include <cstdint>

namespace {

constexpr int ET = 256;
constexpr int EVAL_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(ET) void eval_epe_partial(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       float* __restrict__ part, int B, int Hp, int Wp, int Hg, int Wg,
                                                       int ch, int cw, float maxdisp) {
    __shared__ float sm[6][ET / 64];
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // sum|e|, sum_non, sum_true, n, n_non, n_true
    const long long n = (long long)B * ch * cw;
    for (long long i = (long long)blockIdx.x * ET + threadIdx.x; i < n; i += (long long)gridDim.x * ET) {
        const int x = (int)(i % cw);
        const long long r = i / cw;
        const int y = (int)(r % ch), b = (int)(r / ch);
        const float d = gt[((size_t)b * Hg + y) * Wg + x];
        const float e = fabsf(pred[((size_t)b * Hp + y) * Wp + x] - d);
        const bool m = d < maxdisp && d >= 0.f;
        const bool in = ((float)x - d) >= 0.f;                // test.py:70-72: `local` is the column index as float
        if (m) { acc[0] += e; acc[3] += 1.f; }
        if (m && in) { acc[1] += e; acc[4] += 1.f; }
        if (m && in && d > 0.f) { acc[2] += e; acc[5] += 1.f; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float v = wave_sum(acc[k]);
        if (lane == 0) sm[k][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = 0.f;
        for (int w = 0; w < ET / 64; ++w) v += sm[threadIdx.x][w];
        part[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

__global__ void eval_epe_final(const float* __restrict__ part, int nblocks, float* __restrict__ out6) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nblocks; ++b)
        for (int k = 0; k < 6; ++k) s[k] += (double)part[(size_t)b * 6 + k];
    for (int k = 0; k < 3; ++k) out6[k] = (float)(s[k] / s[3 + k]);      // empty mask -> NaN like torch.mean of nothing
    for (int k = 3; k < 6; ++k) out6[k] = (float)s[k];
}

inline int eval_blocks(long long n) {
    long long b = (n + ET * 8 - 1) / (ET * 8);
    return (int)(b < 1 ? 1 : (b > EVAL_MAX_BLOCKS ? EVAL_MAX_BLOCKS : b));
}

constexpr int U16_MAXB = 32;
struct Sizes { int h[U16_MAXB], w[U16_MAXB]; };

// numpy's float32 -> uint16 cast on the reference's host (x86-64, gcc): cvttss2si to a 32-bit integer, low 16 bits kept;
// values outside the int32 range and NaN give the "integer indefinite" 0x80000000, i.e. 0.  Disparities * 256 of this
// network lie in [0, 48128], far inside; the edge cases are pinned by the golden anyway.
__device__ __forceinline__ unsigned short f32_to_u16_c(float v) {
    if (!(v > -2147483904.0f && v < 2147483648.0f)) return 0;
    return (unsigned short)((unsigned)(int)truncf(v) & 0xffffu);
}

__global__ __launch_bounds__(256) void disp_to_u16(const float* __restrict__ pred, unsigned short* __restrict__ out, Sizes sz,
                                                   int Hp, int Wp, int Ho, int Wo, float scale, int b0) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, bl = blockIdx.z, b = b0 + bl;
    if (x >= Wo) return;
    const int h = sz.h[bl], w = sz.w[bl];
    unsigned short v = 0;
    if (y < h && x < w) v = f32_to_u16_c(pred[((size_t)b * Hp + (Hp - h + y)) * Wp + (Wp - w + x)] * scale);
    out[((size_t)b * Ho + y) * Wo + x] = v;
}

// ---- KITTI validation (eval_kitti.py:84-103) --------------------------------------------------------------------------------
// A workgroup walks spans of KSPAN consecutive pixels of ONE sample (blockIdx.y), so the per-sample rows and the batch row come
// from the same partials: KP words per (sample, workgroup) -- two fp32 error sums (mask, mask_non) and three integer counts
// (mask, mask_non, good).  mask_true is mask_non in the reference, so its column is a copy and costs no accumulator.
constexpr int KT = 256, KSPAN = KT * 8, KITTI_MAX_BLOCKS = 256, KP = 5;

__device__ __forceinline__ void kitti_pixel(float p, float d, unsigned x, float maxdisp, float& s, float& s_non, unsigned& n,
                                            unsigned& n_non, unsigned& n_good) {
    const float e = fabsf(p - d);
    const bool m = d < maxdisp && 0.f < d;
    if (m) { s += e; n += 1u; n_good += (e < 3.f || e < 0.05f * d) ? 1u : 0u; }      // a NaN error is in the sum, never good
    const float local = (float)x;                                                   // eval_kitti.py:84: the column as a float
    if (m && local - d >= 0.f) { s_non += e; n_non += 1u; }
}

// VEC: W % 4 == 0 and both bases 16-byte aligned, so a float4 never straddles a row or a sample.  hw = H * W < 2^31.  Both forms
// give a thread the same four consecutive pixels in the same order, so the fp32 sums -- and with them the whole row -- do not depend
// on the load width: the result is a function of the values, not of where they lie.
template <bool VEC>
__global__ __launch_bounds__(KT) void eval_kitti_partial(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         unsigned* __restrict__ part, unsigned hw, unsigned W, float maxdisp) {
    __shared__ float sf[2][KT / 64];
    __shared__ unsigned sc[3][KT / 64];
    const float* p = pred + (size_t)blockIdx.y * hw;
    const float* g = gt + (size_t)blockIdx.y * hw;
    float s = 0.f, s_non = 0.f;
    unsigned n = 0, n_non = 0, n_good = 0;
    for (unsigned s0 = blockIdx.x * KSPAN; s0 < hw; s0 += gridDim.x * KSPAN) {
#pragma unroll
        for (int k = 0; k < KSPAN / (4 * KT); ++k) {
            const unsigned i = s0 + (k * KT + threadIdx.x) * 4;
            if (VEC) {
                if (i < hw) {
                    const float4 pv = *reinterpret_cast<const float4*>(p + i), dv = *reinterpret_cast<const float4*>(g + i);
                    const unsigned x = i % W;
                    kitti_pixel(pv.x, dv.x, x, maxdisp, s, s_non, n, n_non, n_good);
                    kitti_pixel(pv.y, dv.y, x + 1, maxdisp, s, s_non, n, n_non, n_good);
                    kitti_pixel(pv.z, dv.z, x + 2, maxdisp, s, s_non, n, n_non, n_good);
                    kitti_pixel(pv.w, dv.w, x + 3, maxdisp, s, s_non, n, n_non, n_good);
                }
            } else {
#pragma unroll
                for (unsigned j = 0; j < 4; ++j)
                    if (i + j < hw) kitti_pixel(p[i + j], g[i + j], (i + j) % W, maxdisp, s, s_non, n, n_non, n_good);
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    s = wave_sum(s); s_non = wave_sum(s_non);
    n = wave_sum(n); n_non = wave_sum(n_non); n_good = wave_sum(n_good);
    if (lane == 0) { sf[0][wave] = s; sf[1][wave] = s_non; sc[0][wave] = n; sc[1][wave] = n_non; sc[2][wave] = n_good; }
    __syncthreads();
    if (threadIdx.x < KP) {
        unsigned v;
        if (threadIdx.x < 2) {
            float f = 0.f;
            for (int w = 0; w < KT / 64; ++w) f += sf[threadIdx.x][w];
            v = __float_as_uint(f);
        } else {
            v = 0;
            for (int w = 0; w < KT / 64; ++w) v += sc[threadIdx.x - 2][w];
        }
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * KP + threadIdx.x] = v;
    }
}

// eval_kitti.py:101-103 keeps its two sums as fp32 sums of ones and forms 100 - good / total * 100 in fp32; the same three
// roundings here (uncontracted), from the exact counts.  0 / 0 -> NaN.
__device__ __forceinline__ float kitti_err3(unsigned long long good, unsigned long long total) {
#pragma clang fp contract(off)
    const float q = (float)good / (float)total;
    const float q100 = q * 100.f;
    return 100.f - q100;
}

// [loss, loss_non, loss_true, loss_3, n_mask, n_non, n_true, n_good]
__device__ __forceinline__ void kitti_row(float* __restrict__ out, double s, double s_non, unsigned long long n,
                                          unsigned long long n_non, unsigned long long n_good) {
    const float m = (float)(s / (double)n), m_non = (float)(s_non / (double)n_non);      // empty mask -> NaN
    out[0] = m; out[1] = m_non; out[2] = m_non; out[3] = kitti_err3(n_good, n);
    out[4] = (float)n; out[5] = (float)n_non; out[6] = (float)n_non; out[7] = (float)n_good;
}

// One workgroup of min(B, 16) waves; a wave takes samples wave, wave + nwaves, ...: lane l adds the partials of workgroups
// l, l + 64, ... (sums in fp64, counts in 64-bit integers), then a fixed-order butterfly as in loss.hip.  Thread 0 then adds
// the per-sample totals in sample order: no atomics, the same bits every run.
__global__ __launch_bounds__(1024) void eval_kitti_final(const unsigned* __restrict__ part, int nbx, int B, float* __restrict__ out8,
                                                         float* __restrict__ per_sample, unsigned long long* tot) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    for (int b = wave; b < B; b += nwaves) {
        double s = 0, s_non = 0;
        unsigned long long c[3] = {0, 0, 0};
        for (int blk = lane; blk < nbx; blk += 64) {
            const unsigned* q = part + ((size_t)b * nbx + blk) * KP;
            s += (double)__uint_as_float(q[0]);
            s_non += (double)__uint_as_float(q[1]);
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] += q[2 + k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s += __shfl_xor(s, off, 64);
            s_non += __shfl_xor(s_non, off, 64);
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] += __shfl_xor(c[k], off, 64);
        }
        if (lane == 0) {
            if (per_sample) kitti_row(per_sample + (size_t)b * 8, s, s_non, c[0], c[1], c[2]);
            unsigned long long* t = tot + (size_t)b * KP;
            t[0] = (unsigned long long)__double_as_longlong(s);
            t[1] = (unsigned long long)__double_as_longlong(s_non);
            t[2] = c[0]; t[3] = c[1]; t[4] = c[2];
        }
    }
    __syncthreads();                       // the totals written above are visible to thread 0 (same workgroup)
    if (threadIdx.x != 0) return;
    double s = 0, s_non = 0;
    unsigned long long c[3] = {0, 0, 0};
    for (int b = 0; b < B; ++b) {
        const unsigned long long* t = tot + (size_t)b * KP;
        s += __longlong_as_double((long long)t[0]);
        s_non += __longlong_as_double((long long)t[1]);
        c[0] += t[2]; c[1] += t[3]; c[2] += t[4];
    }
    kitti_row(out8, s, s_non, c[0], c[1], c[2]);
}

inline int kitti_blocks(long long hw) {
    const long long b = (hw + KSPAN - 1) / KSPAN;
    return (int)(b > KITTI_MAX_BLOCKS ? KITTI_MAX_BLOCKS : b);
}

inline long long kitti_part_bytes(int B, long long hw) {      // the partials, rounded up to the 8-byte totals behind them
    return ((long long)B * kitti_blocks(hw) * KP * (long long)sizeof(unsigned) + 7) / 8 * 8;
}

}  // namespace

extern "C" long long ecm_eval_epe_scratch_bytes(long long n) {
    return n > 0 ? (long long)eval_blocks(n) * 6 * (long long)sizeof(float) : 0;
}

extern "C" int ecm_eval_epe(const float* pred, const float* gt, float* out6, void* scratch, long long scratch_bytes, int B,
                            int Hp, int Wp, int Hg, int Wg, int crop_h, int crop_w, float maxdisp, void* stream) {
    ECM_CHECK_ARG(pred && gt && out6 && scratch && B > 0 && crop_h > 0 && crop_w > 0);
    ECM_CHECK_ARG(crop_h <= Hp && crop_h <= Hg && crop_w <= Wp && crop_w <= Wg);
    const long long n = (long long)B * crop_h * crop_w;
    if (scratch_bytes < ecm_eval_epe_scratch_bytes(n)) return ECM_ESCRATCH;
    const int nb = eval_blocks(n);
    float* part = static_cast<float*>(scratch);
    hipStream_t st = ecm_stream(stream);
    hipLaunchKernelGGL(eval_epe_partial, dim3(nb), dim3(ET), 0, st, pred, gt, part, B, Hp, Wp, Hg, Wg, crop_h, crop_w, maxdisp);
    hipLaunchKernelGGL(eval_epe_final, dim3(1), dim3(64), 0, st, part, nb, out6);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_disp_to_u16(const float* pred, unsigned short* out, int B, int Hp, int Wp, const int* h, const int* w,
                               int Ho, int Wo, float scale, void* stream) {
    ECM_CHECK_ARG(pred && out && h && w && B > 0 && Hp > 0 && Wp > 0 && Ho > 0 && Wo > 0);
    for (int b = 0; b < B; ++b) ECM_CHECK_ARG(h[b] > 0 && w[b] > 0 && h[b] <= Hp && w[b] <= Wp && h[b] <= Ho && w[b] <= Wo);
    if (Ho > 65535) return ECM_EUNSUP;
    hipStream_t st = ecm_stream(stream);
    for (int b0 = 0; b0 < B; b0 += U16_MAXB) {
        const int nb = B - b0 < U16_MAXB ? B - b0 : U16_MAXB;
        Sizes sz;
        for (int i = 0; i < nb; ++i) { sz.h[i] = h[b0 + i]; sz.w[i] = w[b0 + i]; }
        hipLaunchKernelGGL(disp_to_u16, dim3((Wo + 255) / 256, Ho, nb), dim3(256), 0, st, pred, out, sz, Hp, Wp, Ho, Wo, scale, b0);
    }
    return ECM_LAUNCH_RESULT();
}

extern "C" long long ecm_eval_kitti_scratch_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || B > 65535 || (long long)H * W > 0x7fffffffLL) return 0;   // what ecm_eval_kitti refuses
    return kitti_part_bytes(B, (long long)H * W) + (long long)B * KP * (long long)sizeof(unsigned long long);
}

extern "C" int ecm_eval_kitti(const float* pred, const float* gt, float* out8, float* per_sample, void* scratch,
                              long long scratch_bytes, int B, int H, int W, float maxdisp, void* stream) {
    ECM_CHECK_ARG(pred && gt && out8 && scratch && B >= 1 && H >= 1 && W >= 1);
    ECM_CHECK_ARG(reinterpret_cast<uintptr_t>(scratch) % 8 == 0);
    const long long hw = (long long)H * W;
    if (hw > 0x7fffffffLL || B > 65535) return ECM_EUNSUP;        // 32-bit pixel index inside a sample; blockIdx.y is the sample
    if (scratch_bytes < ecm_eval_kitti_scratch_bytes(B, H, W)) return ECM_ESCRATCH;
    const int nbx = kitti_blocks(hw);
    unsigned* part = static_cast<unsigned*>(scratch);
    unsigned long long* tot = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + kitti_part_bytes(B, hw));
    hipStream_t st = ecm_stream(stream);
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(pred) % 16 == 0 && reinterpret_cast<uintptr_t>(gt) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(eval_kitti_partial<true>, dim3(nbx, B), dim3(KT), 0, st, pred, gt, part, (unsigned)hw, (unsigned)W, maxdisp);
    else
        hipLaunchKernelGGL(eval_kitti_partial<false>, dim3(nbx, B), dim3(KT), 0, st, pred, gt, part, (unsigned)hw, (unsigned)W, maxdisp);
    hipLaunchKernelGGL(eval_kitti_final, dim3(1), dim3(64 * (B < 16 ? B : 16)), 0, st, part, nbx, B, out8, per_sample, tot);
    return ECM_LAUNCH_RESULT();
}
