// Opt-in bf16 inference of the cmf refinement decoder (ops.decoder_dtype): the two forward-only kernels that
// bf16_encoder.hip and gn3d.hip do not already provide.  Reference layers: super_resolution_refinement, cmf.py:227-264.
//
// A. ConvTranspose2d(Ci, Co, 3, stride 2, padding 1, output_padding 1, bias) (cmf.py:236-239) on a bf16 NCHW x, bf16 y.
//    Output (2i+py, 2j+px) reads the inputs (i+dy, j+dx), dy, dx in {0, 1}: tap k along an axis has phase p = (k != 1) and
//    offset d = (k == 0), so the four phases are stride-1 convolutions over the input grid with 1, 2, 2 and 4 of the nine
//    taps.  A workgroup stages ONE halo tile of (4+1) x (32+1) input positions per 16-channel chunk -- [position][16 channels]
//    in LDS next to the chunk's [tap][Co][16] weight slice, through the staging pipeline of bf16_conv2d.h that conv2d_bf16
//    (bf16_encoder.hip) runs on as well -- and computes all four phases from it on
//    v_mfma_f32_32x32x16_bf16:  D[co][input column] += A[co][16 channels of one tap] * B[16 channels][input column + dx].
//    Each of the four waves owns one input row: 4 phases x Co/32 accumulator tiles, preset with the fp32 bias.
//    A lane owns input column j, hence the px = 0 and px = 1 outputs 2j and 2j+1 of a row: they are rounded once and stored
//    as one 4-byte pair, so a wave writes 128 contiguous bytes per (channel, output row).
// B. conv_out: relu(Conv2d(Ci, 1, 3, 1, 1, bias)(x)) (cmf.py:259-264) on a bf16 x, fp32 y.  HBM-bound (Ci bf16 planes in, one
//    fp32 plane out), on the vector ALU with no LDS staging of x and no barrier in the channel loop: a lane owns 8 adjacent
//    columns of 4 output rows, reads the 6 input rows of a channel as 16-byte loads (a wave reads 1 KB of a row at once),
//    takes the two columns beside its segment from its neighbour lanes, widens bf16 -> fp32 in registers and accumulates in
//    fp32.  Every load is branch-free (load8 of bf16_conv2d.h: an outside column loads a valid address and is zeroed by a
//    select), so a channel's 6 + 6 loads are issued back to back and waited for once; the latency is covered by the other
//    waves of the SIMD (167 VGPRs: 3 waves), not by a register pipeline -- two channels in flight per wave took 218-256
//    VGPRs.  The 9*Ci weights are rounded to bf16 once into LDS and read from there at a wave-uniform address.
// No atomics: each output is one thread's fixed-order sum, so results are bit-reproducible.
#include "common.h"
#include "bf16_conv2d.h"

namespace {

// ---- A: transposed convolution ------------------------------------------------------------------------------------------------
constexpr int DTW = 32, DTH = 4;                       // input columns / rows per workgroup (one row per wave)
constexpr int DIWP = 40, DHR = DTH + 1;                // window columns (33 needed, widened to whole 8-column segments), halo rows
template <int COT>
using DecStage = Stage2d<DHR, DIWP, 9, COT>;           // 200 staging units: one per thread

template <int COT, bool VEC>
__global__ __launch_bounds__(256, 2) void deconv2d_bf16(const u16* __restrict__ x, const u16* __restrict__ wp,
                                                        const float* __restrict__ bias, u16* __restrict__ y, int Ci, int H,
                                                        int W, int tiles_h, int tiles_w) {
    constexpr int COP = COT * 32;
    extern __shared__ __attribute__((aligned(16))) char smem_d[];

    int bid = ecm_xcd_tile(blockIdx.x, gridDim.x);
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int b = bid / tiles_h;
    const int i0 = th * DTH, j0 = tw * DTW;                                        // window origin (j0 % 8 == 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const size_t HW = (size_t)H * W;
    const u16* xb = x + (size_t)b * Ci * HW;

    // accumulators [phase py*2+px][channel tile], preset with the bias of the register's channel
    f32x16 acc[4][COT];
#pragma unroll
    for (int ct = 0; ct < COT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float bv = bias[ct * 32 + mfma32_row(i, half)];
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[p][ct][i] = bv;
        }
    const int rbase = (wave * DIWP + l31) * 2 + half;                              // B fragment of offset (0, 0)

    // the weight image has Co == COP, so the workgroup's slice is the whole (contiguous) chunk
    stage2d_run<DecStage<COT>, VEC>(smem_d, xb, Ci, H, W, i0, j0, wp, COP, 0, [&](const uint4* Xs, const uint4* Ws) __attribute__((always_inline)) {
        bf16x8 bv[2][2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) bv[dy][dx] = __builtin_bit_cast(bf16x8, Xs[rbase + (dy * DIWP + dx) * 2]);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t % 3;
            const int p = (ky != 1) * 2 + (kx != 1);
#pragma unroll
            for (int ct = 0; ct < COT; ++ct) {
                const bf16x8 a = __builtin_bit_cast(bf16x8, Ws[(t * COP + ct * 32 + l31) * 2 + half]);
                acc[p][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv[ky == 0][kx == 0], acc[p][ct], 0, 0, 0);
            }
        }
    });

    // epilogue: lane = input column, register i = output channel mfma32_row(i, half) of the tile
    const int i = i0 + wave, j = j0 + l31;
    if (i >= H || j >= W) return;
    const int Wo = 2 * W;
    const size_t HWo = 4 * HW;
    u16* yb = y + (size_t)b * COP * HWo + (size_t)(2 * i) * Wo + 2 * j;
#pragma unroll
    for (int ct = 0; ct < COT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            u16* dst = yb + (size_t)(ct * 32 + mfma32_row(r, half)) * HWo;
#pragma unroll
            for (int py = 0; py < 2; ++py)
                *reinterpret_cast<unsigned*>(dst + py * Wo) = (unsigned)f2bf(acc[py * 2][ct][r]) | ((unsigned)f2bf(acc[py * 2 + 1][ct][r]) << 16);
        }
}

template <int COT>
int launch_dec(const u16* x, const u16* wp, const float* bias, u16* y, int B, int Ci, int H, int W, void* stream) {
    const int th = (H + DTH - 1) / DTH, tw = (W + DTW - 1) / DTW;
    const long long nb = (long long)B * th * tw;
    if (nb > 0x7fffffffLL) return ECM_EUNSUP;
    return stage2d_launch(deconv2d_bf16<COT, true>, deconv2d_bf16<COT, false>, W % 8 == 0, dim3((unsigned)nb), DecStage<COT>::LDS_BYTES,
                          stream, x, wp, bias, y, Ci, H, W, th, tw);
}

// ---- B: one output channel ----------------------------------------------------------------------------------------------------
constexpr int C1R = 4;                                 // output rows per lane
constexpr int C1W = 64 * 8;                            // columns per wave: 8 per lane
constexpr int C1MAXW = 9 * 1024;                       // weights held in LDS: Ci <= 1024 (36 KB, under the default limit)

template <bool VEC>
__global__ __launch_bounds__(256) void conv2d_c1_bf16(const u16* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y, int Ci, int H, int W,
                                                      int tiles_h, int tiles_w) {
    extern __shared__ __attribute__((aligned(16))) float ws[];                      // 9 * Ci weights
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 9 * Ci; i += 256) ws[i] = bf2f(f2bf(w[i]));             // the weight's one rounding
    __syncthreads();

    int bid = ecm_xcd_tile(blockIdx.x, gridDim.x);
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int b = bid / tiles_h;
    const int r0 = (th * 4 + wave) * C1R;                                          // first output row of the wave
    const int c0 = tw * C1W + lane * 8;                                            // first column of the lane
    if (r0 >= H) return;                                                           // wave-uniform; no barrier follows
    const size_t HW = (size_t)H * W;
    const u16* xb = x + (size_t)b * Ci * HW;

    // the columns beside the segment come from the neighbour lanes; lanes 0 and 63 read theirs from memory
    const bool edge = lane == 0 || lane == 63;
    const int ec = lane == 0 ? c0 - 1 : c0 + 8;
    const bool ecok = ec >= 0 && ec < W;
    unsigned vok[C1R + 2];                                                         // which of the lane's 8 columns exist, per input row
    bool eok[C1R + 2];
    int voff[C1R + 2], eoff[C1R + 2];
#pragma unroll
    for (int r = 0; r < C1R + 2; ++r) {
        const int gy = r0 - 1 + r;
        const bool rok = gy >= 0 && gy < H;
        vok[r] = mask8<VEC>(rok, c0, W);
        voff[r] = rok ? gy * W + c0 : 0;
        eok[r] = rok && edge && ecok;
        eoff[r] = eok[r] ? gy * W + ec : 0;
    }

    float acc[C1R][8];
#pragma unroll
    for (int r = 0; r < C1R; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;

    for (int ci = 0; ci < Ci; ++ci) {
        const u16* plane = xb + (size_t)ci * HW;
        u32x4 v[C1R + 2];
        unsigned ev[C1R + 2];
#pragma unroll
        for (int r = 0; r < C1R + 2; ++r) {
            v[r] = load8<VEC>(plane, voff[r], vok[r]);
            const unsigned t = plane[eoff[r]];
            ev[r] = eok[r] ? t : 0u;
        }
        float wk[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wk[t] = ws[ci * 9 + t];
#pragma unroll
        for (int r = 0; r < C1R + 2; ++r) {
            const unsigned lw = __shfl_up(v[r][3], 1, 64), rw = __shfl_down(v[r][0], 1, 64);
            float f[10];
            f[0] = __builtin_bit_cast(float, lane == 0 ? ev[r] << 16 : lw & 0xffff0000u);
            f[9] = __builtin_bit_cast(float, lane == 63 ? ev[r] << 16 : rw << 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f[1 + 2 * k] = __builtin_bit_cast(float, v[r][k] << 16);
                f[2 + 2 * k] = __builtin_bit_cast(float, v[r][k] & 0xffff0000u);
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int ro = r - ky;                                             // input row r feeds output row r - ky with tap row ky
                if (ro < 0 || ro >= C1R) continue;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    acc[ro][c] = __builtin_fmaf(wk[ky * 3 + 2], f[c + 2], __builtin_fmaf(wk[ky * 3 + 1], f[c + 1], __builtin_fmaf(wk[ky * 3], f[c], acc[ro][c])));
            }
        }
    }

    const float bs = bias[0];
    float* yb = y + (size_t)b * HW;
#pragma unroll
    for (int r = 0; r < C1R; ++r) {
        const int gy = r0 + r;
        if (gy >= H) break;
        float o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = fmaxf(acc[r][c] + bs, 0.f);
        float* dst = yb + (size_t)gy * W + c0;
        if (VEC) {
            if (c0 < W) {
                *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(dst + 4) = make_float4(o[4], o[5], o[6], o[7]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c0 + c < W) dst[c] = o[c];
        }
    }
}

}  // namespace

extern "C" long long ecm_deconv2d_bf16_packed_elems(int Ci, int Co) {
    return (Ci > 0 && Ci % KC == 0 && (Co == 32 || Co == 64)) ? (long long)Ci * 9 * Co : 0;
}

extern "C" int ecm_deconv2d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0);
    const long long n = ecm_deconv2d_bf16_packed_elems(Ci, Co);
    if (n == 0) return ECM_EUNSUP;
    return pack_weight_2d(w, packed, Ci, Co, 9, 1, stream);
}

extern "C" int ecm_deconv2d_k3s2_bias_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, const float* bias,
                                               unsigned short* y, int B, int Ci, int Co, int H, int W, void* stream) {
    ECM_CHECK_ARG(x && wpacked && bias && y && B > 0 && Ci > 0 && Co > 0 && H > 0 && W > 0);
    if (Ci % KC != 0 || (Co != 32 && Co != 64)) return ECM_EUNSUP;
    // element offsets inside one sample's planes stay 32-bit
    if ((long long)Ci * H * W >= 0x7fffffffLL || (long long)Co * 4 * H * W >= 0x7fffffffLL) return ECM_EUNSUP;
    if (Co == 64) return launch_dec<2>(x, wpacked, bias, y, B, Ci, H, W, stream);
    return launch_dec<1>(x, wpacked, bias, y, B, Ci, H, W, stream);
}

extern "C" int ecm_conv2d_c1_bf16_fwd(const unsigned short* x, const float* w, const float* bias, float* y, int B, int Ci, int H,
                                      int W, void* stream) {
    ECM_CHECK_ARG(x && w && bias && y && B > 0 && Ci > 0 && H > 0 && W > 0);
    if (Ci % KC != 0 || 9 * Ci > C1MAXW || (long long)H * W >= 0x7fffffffLL) return ECM_EUNSUP;
    const int th = (H + 4 * C1R - 1) / (4 * C1R), tw = (W + C1W - 1) / C1W;
    const long long nb = (long long)B * th * tw;
    if (nb > 0x7fffffffLL) return ECM_EUNSUP;
    if (W % 8 == 0)
        hipLaunchKernelGGL((conv2d_c1_bf16<true>), dim3((unsigned)nb), dim3(256), 9 * Ci * sizeof(float), ecm_stream(stream), x, w, bias, y, Ci, H, W, th, tw);
    else
        hipLaunchKernelGGL((conv2d_c1_bf16<false>), dim3((unsigned)nb), dim3(256), 9 * Ci * sizeof(float), ecm_stream(stream), x, w, bias, y, Ci, H, W, th, tw);
    return ECM_LAUNCH_RESULT();
}
