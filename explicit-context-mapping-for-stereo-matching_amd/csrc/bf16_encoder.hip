// Opt-in bf16 inference of the 2-D feature encoder (ops.encoder_dtype): forward-only kernels on bf16 NCHW maps with fp32
// accumulation.  Reference layers: convbn / the 1x1 projections of feature_extraction (cmfsm.py:36-46, 126-236).
//
// Convolution (3x3 with stride 1|2 and dilation 1|2|4, padding = dilation; 1x1 with stride 1|2, no padding) is ONE
// implicit-GEMM body on v_mfma_f32_32x32x16_bf16:  D[co][pixel] += sum_k A[co][k] * B[k][pixel].
//   k-step = ONE tap x 16 input channels: lane half h (= lane >> 5) takes channels 8h .. 8h+7 of the chunk, so one
//   16-byte LDS read gives a lane its whole fragment; no tap slot is padding.  How the [position][16 channels] halo tile and
//   the [tap][co][16 channels] weight slice of a chunk reach LDS (16-byte row loads, the transposing channel-pair write, the
//   double-buffered chunk loop) is bf16_conv2d.h; this file is the tile geometry, the tap loop, the epilogue and the dispatch.
//   The output type is a template parameter: bf16 inside the encoder, fp32 for the layers whose result leaves it.
// No atomics: each output is one workgroup's fixed-order sum, so results are bit-reproducible.
// The GroupNorm that ends the region (bf16 in, fp32 out plus an optional bf16 copy) is gn3d.hip's ecm_gn3d_apply_bf16_f32.
#include "common.h"
#include "bf16_conv2d.h"

namespace {

__device__ __forceinline__ void store_out(u16* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void store_out(float* p, float v) { *p = v; }

constexpr int TW = 32;          // output pixels along w per MFMA row (the B operand's 32 columns)

// KS: kernel size (1 or 3), S: stride, DL: dilation, NT: output rows per wave (4 waves: TH = 4*NT rows per workgroup)
template <int KS, int S, int DL, int NT>
struct Geo2 {
    static constexpr int KK = KS * KS;
    static constexpr int PAD = DL * (KS - 1) / 2;
    static constexpr int TH = 4 * NT;
    static constexpr int HR = S * (TH - 1) + DL * (KS - 1) + 1;                    // halo rows
    static constexpr int XOFF = PAD ? 8 - PAD : 0;                                // first needed column inside the 8-aligned window
    static constexpr int IWP = (XOFF + S * (TW - 1) + DL * (KS - 1) + 1 + 7) / 8 * 8;   // window columns (multiple of 8)
    static_assert(PAD <= 8, "window origin");
};

template <int KS, int S, int DL, int NT, int COT>
using EncStage = Stage2d<Geo2<KS, S, DL, NT>::HR, Geo2<KS, S, DL, NT>::IWP, Geo2<KS, S, DL, NT>::KK, COT>;

template <int KS, int S, int DL, int NT, int COT, bool VEC, class OutT>
__global__ __launch_bounds__(256, 2) void conv2d_bf16(const u16* __restrict__ x, const u16* __restrict__ wp,
                                                      OutT* __restrict__ y, int Ci, int Co, int H, int W, int Ho, int Wo,
                                                      int tiles_h, int tiles_w) {
    using G = Geo2<KS, S, DL, NT>;
    constexpr int KK = G::KK, TH = G::TH, IWP = G::IWP, COP = COT * 32;
    extern __shared__ __attribute__((aligned(16))) char smem_e[];

    int bid = ecm_xcd_tile(blockIdx.x, gridDim.x);
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int b = bid / tiles_h;
    const int cb = blockIdx.y;                                                     // output-channel block of COP
    const int oh0 = th * TH, ow0 = tw * TW;
    const int gy0 = S * oh0 - G::PAD, gx0 = S * ow0 - G::PAD - G::XOFF;           // window origin (gx0 % 8 == 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const size_t HW = (size_t)H * W;
    const u16* xb = x + (size_t)b * Ci * HW;

    f32x16 acc[NT][COT];
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
        for (int ct = 0; ct < COT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[r][ct][i] = 0.f;
    int rbase[NT];                                                                 // B fragment: position of tap (0,0), then the half
#pragma unroll
    for (int r = 0; r < NT; ++r) rbase[r] = ((S * (wave * NT + r)) * IWP + S * l31 + G::XOFF) * 2 + half;

    stage2d_run<EncStage<KS, S, DL, NT, COT>, VEC>(smem_e, xb, Ci, H, W, gy0, gx0, wp, Co, cb,
                                                   [&](const uint4* Xs, const uint4* Ws) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < KK; ++t) {
            const int kh = t / KS, kw = t % KS;
            const int toff = (kh * DL * IWP + kw * DL) * 2;
            bf16x8 a[COT];
#pragma unroll
            for (int ct = 0; ct < COT; ++ct) a[ct] = __builtin_bit_cast(bf16x8, Ws[(t * COP + ct * 32 + l31) * 2 + half]);
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                const bf16x8 bv = __builtin_bit_cast(bf16x8, Xs[rbase[r] + toff]);
#pragma unroll
                for (int ct = 0; ct < COT; ++ct)
                    acc[r][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ct], bv, acc[r][ct], 0, 0, 0);
            }
        }
    });

    // epilogue: lane = pixel l31 of the row, register i = output channel mfma32_row(i, half) of the tile
    const size_t HWo = (size_t)Ho * Wo;
    OutT* yb = y + ((size_t)b * Co + cb * COP) * HWo;
    const int ow = ow0 + l31;
    if (ow >= Wo) return;
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        const int oh = oh0 + wave * NT + r;
        if (oh >= Ho) continue;
        OutT* dst = yb + (size_t)oh * Wo + ow;
#pragma unroll
        for (int ct = 0; ct < COT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) store_out(dst + (size_t)(ct * 32 + mfma32_row(i, half)) * HWo, acc[r][ct][i]);
    }
}

template <int KS, int S, int DL, int NT, int COT, class OutT>
int launch_enc(const u16* x, const u16* wp, OutT* y, int B, int Ci, int Co, int H, int W, int Ho, int Wo, void* stream) {
    constexpr int TH = 4 * NT;
    const int th = (Ho + TH - 1) / TH, tw = (Wo + TW - 1) / TW;
    const long long nb = (long long)B * th * tw;
    if (nb > 0x7fffffffLL || Co / (COT * 32) > 65535) return ECM_EUNSUP;
    return stage2d_launch(conv2d_bf16<KS, S, DL, NT, COT, true, OutT>, conv2d_bf16<KS, S, DL, NT, COT, false, OutT>, W % 8 == 0,
                          dim3((unsigned)nb, (unsigned)(Co / (COT * 32))), EncStage<KS, S, DL, NT, COT>::LDS_BYTES, stream, x, wp, y,
                          Ci, Co, H, W, Ho, Wo, th, tw);
}

// output channels per workgroup: up to 64 (3x3: the weight slice of a chunk is 9 taps deep), 128 for a stride-1 1x1
template <int KS, int S, int DL, int NT, class OutT>
int launch_co(const u16* x, const u16* wp, OutT* y, int B, int Ci, int Co, int H, int W, int Ho, int Wo, void* stream) {
    if constexpr (KS == 1 && S == 1)
        if (Co % 128 == 0) return launch_enc<KS, S, DL, NT, 4, OutT>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    if (Co % 64 == 0) return launch_enc<KS, S, DL, NT, 2, OutT>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    return launch_enc<KS, S, DL, NT, 1, OutT>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
}

template <class OutT>
int dispatch(const u16* x, const u16* wp, OutT* y, int B, int Ci, int Co, int H, int W, int k, int stride, int dil, void* stream) {
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if (k == 3 && stride == 1 && dil == 1) return launch_co<3, 1, 1, 2>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    if (k == 3 && stride == 1 && dil == 2) return launch_co<3, 1, 2, 2>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    if (k == 3 && stride == 1 && dil == 4) return launch_co<3, 1, 4, 1>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    if (k == 3 && stride == 2 && dil == 1) return launch_co<3, 2, 1, 1>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    if (k == 1 && stride == 1 && dil == 1) return launch_co<1, 1, 1, 2>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    if (k == 1 && stride == 2 && dil == 1) return launch_co<1, 2, 1, 2>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);
    return ECM_EUNSUP;
}

}  // namespace

extern "C" long long ecm_conv2d_bf16_packed_elems(int Ci, int Co, int k) {
    return (Ci > 0 && Co > 0 && Ci % KC == 0 && (k == 1 || k == 3)) ? (long long)Ci * k * k * Co : 0;
}

extern "C" int ecm_conv2d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int k, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0);
    if ((k != 1 && k != 3) || Ci % KC != 0) return ECM_EUNSUP;
    return pack_weight_2d(w, packed, Ci, Co, k * k, 0, stream);
}

extern "C" int ecm_conv2d_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, void* y, int B, int Ci, int Co,
                                   int H, int W, int k, int stride, int dil, int out_f32, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && H > 0 && W > 0);
    if ((k != 1 && k != 3) || (stride != 1 && stride != 2) || dil < 1) return ECM_EUNSUP;
    if (Ci % KC != 0 || Co % 32 != 0) return ECM_EUNSUP;
    // element offsets inside one sample's planes stay 32-bit
    const long long Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long long)Ci * H * W >= 0x7fffffffLL || (long long)Co * Ho * Wo >= 0x7fffffffLL) return ECM_EUNSUP;
    if (out_f32) return dispatch<float>(x, wpacked, static_cast<float*>(y), B, Ci, Co, H, W, k, stride, dil, stream);
    return dispatch<u16>(x, wpacked, static_cast<u16*>(y), B, Ci, Co, H, W, k, stride, dil, stream);
}
