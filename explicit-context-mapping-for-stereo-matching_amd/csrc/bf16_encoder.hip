// Opt-in bf16 inference of the 2-D feature encoder (ops.encoder_dtype): forward-only kernels on bf16 NCHW maps with fp32
// accumulation.  Reference layers: convbn / the 1x1 projections of feature_extraction (cmfsm.py:36-46, 126-236).
//
// Convolution (3x3 with stride 1|2 and dilation 1|2|4, padding = dilation; 1x1 with stride 1|2, no padding) is ONE
// implicit-GEMM body on v_mfma_f32_32x32x16_bf16:  D[co][pixel] += sum_k A[co][k] * B[k][pixel].
//   k-step = ONE tap x 16 input channels: lane half h (= lane >> 5) takes channels 8h .. 8h+7 of the chunk, so one
//   16-byte LDS read gives a lane its whole fragment.  The halo tile of a 16-channel chunk sits in LDS as
//   [position][16 channels] and the chunk's weight slice as [tap][co][16 channels]; no tap slot is padding.
//   Staging reads whole rows of each channel plane with 16-byte loads (8 positions of one channel; the window is widened
//   to 8-aligned columns), and a thread that holds the same 8 positions of two channels writes them as 8 channel-pair
//   words -- the [channel][position] -> [position][channel] transpose happens in that write.  Rows of a width that is not
//   a multiple of 8 are not 16-byte aligned: that case stages the same window with 2-byte loads.
//   The LDS tile is double-buffered: chunk c+1 is written into the other buffer after chunk c's MFMAs, and its global
//   loads (issued one chunk earlier) are in flight under them; one barrier per chunk.
//   The output type is a template parameter: bf16 inside the encoder, fp32 for the layers whose result leaves it.
// No atomics: each output is one workgroup's fixed-order sum, so results are bit-reproducible.
// The GroupNorm that ends the region (bf16 in, fp32 out plus an optional bf16 copy) is gn3d.hip's ecm_gn3d_apply_bf16_f32.
#include "common.h"
#include "bf16.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));     // a native vector: promoted to registers, unlike uint4 copies

__device__ __forceinline__ void store_out(u16* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void store_out(float* p, float v) { *p = v; }

constexpr int TW = 32;          // output pixels along w per MFMA row (the B operand's 32 columns)
constexpr int KC = 16;          // input channels per k-step

// KS: kernel size (1 or 3), S: stride, DL: dilation, NT: output rows per wave (4 waves: TH = 4*NT rows per workgroup)
template <int KS, int S, int DL, int NT>
struct Geo2 {
    static constexpr int KK = KS * KS;
    static constexpr int PAD = DL * (KS - 1) / 2;
    static constexpr int TH = 4 * NT;
    static constexpr int HR = S * (TH - 1) + DL * (KS - 1) + 1;                    // halo rows
    static constexpr int XOFF = PAD ? 8 - PAD : 0;                                // first needed column inside the 8-aligned window
    static constexpr int IWP = (XOFF + S * (TW - 1) + DL * (KS - 1) + 1 + 7) / 8 * 8;   // window columns (multiple of 8)
    static constexpr int NSEG = IWP / 8;
    static constexpr int NPOS = HR * IWP;
    static constexpr int NU = (KC / 2) * HR * NSEG;                               // staging units: channel pair x row x segment
    static constexpr int UPT = (NU + 255) / 256;
    static constexpr int HRA = (UPT * 256 + 8 * NSEG - 1) / (8 * NSEG);           // rows allocated: every thread's units land
    static constexpr int NPOSA = HRA * IWP;                                       // in LDS, so the staging needs no branch
    static_assert(PAD <= 8, "window origin");
};

template <int KS, int S, int DL, int NT, int COT>
constexpr int enc_lds_bytes() {
    using G = Geo2<KS, S, DL, NT>;
    return 2 * (G::NPOSA * KC * 2 + (G::KK * COT * 64 + 255) / 256 * 256 * 16);   // two buffers of (halo + weight slice)
}

template <int KS, int S, int DL, int NT, int COT, bool VEC, class OutT>
__global__ __launch_bounds__(256, 2) void conv2d_bf16(const u16* __restrict__ x, const u16* __restrict__ wp,
                                                      OutT* __restrict__ y, int Ci, int Co, int H, int W, int Ho, int Wo,
                                                      int tiles_h, int tiles_w) {
    using G = Geo2<KS, S, DL, NT>;
    constexpr int KK = G::KK, TH = G::TH, IWP = G::IWP, NSEG = G::NSEG, UPT = G::UPT;
    constexpr int COP = COT * 32;
    constexpr int XBYTES = G::NPOSA * KC * 2, WQ = KK * COP * 2;                  // halo bytes, weight uint4s per buffer
    constexpr int WPT = (WQ + 255) / 256;
    constexpr int BUF = XBYTES + WPT * 256 * 16;                                  // the weight area rounded up to whole passes
    static_assert(BUF * 2 == enc_lds_bytes<KS, S, DL, NT, COT>(), "LDS size");
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

    // staging unit u: channel pair cp (fastest), segment j, row r
    int uoff[UPT], ulds[UPT];
    unsigned uok[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
        const int u = tid + k * 256;
        const int cp = u & 7, j = (u >> 3) % NSEG, r = (u >> 3) / NSEG;
        const int gy = gy0 + r, gx = gx0 + 8 * j;
        const bool in = u < G::NU;
        uok[k] = 0;
        if (in && (unsigned)gy < (unsigned)H) {
            if (VEC) uok[k] = (unsigned)gx < (unsigned)W ? 0xffu : 0u;              // W % 8 == 0: a segment is all in or all out
            else
                for (int e = 0; e < 8; ++e) uok[k] |= ((unsigned)(gx + e) < (unsigned)W ? 1u : 0u) << e;
        }
        uoff[k] = gy * W + gx;                                                     // element offset inside a channel plane
        ulds[k] = ((r * IWP + 8 * j) * KC + 2 * cp) * 2;                           // byte offset of position 0, channel 2cp
    }
    uint4 xr[UPT][2];
    u32x4 wr[WPT];
    const int nchunks = Ci / KC;

    auto fetch = [&](int chunk) __attribute__((always_inline)) {
        const int c0 = chunk * KC;
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const int cp = (tid + k * 256) & 7;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u16* src = xb + (size_t)(c0 + 2 * cp + q) * HW;
                // branch-free: an outside position loads the plane's first element and is zeroed by a select
                if (VEC) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + (uok[k] ? uoff[k] : 0));
                    xr[k][q] = uok[k] ? v : make_uint4(0, 0, 0, 0);
                } else {
                    unsigned v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool ok = (uok[k] >> e) & 1u;
                        const unsigned t = src[ok ? uoff[k] + e : 0];
                        v[e] = ok ? t : 0u;
                    }
                    xr[k][q] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
                }
            }
        }
        // the chunk's weight slice [tap][COP][16] (L2-resident: every workgroup reads the same few KB)
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(wp);
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int e = min(tid + i * 256, WQ - 1);                              // branch-free: the tail re-reads the last vector
            const int hh = e & 1, col = (e >> 1) % COP, t = (e >> 1) / COP;
            wr[i] = wsrc[(((size_t)chunk * KK + t) * Co + cb * COP + col) * 2 + hh];
        }
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
        char* base = smem_e + buf * BUF;
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const unsigned a[4] = {xr[k][0].x, xr[k][0].y, xr[k][0].z, xr[k][0].w};
            const unsigned c[4] = {xr[k][1].x, xr[k][1].y, xr[k][1].z, xr[k][1].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned lo = (a[e >> 1] >> (16 * (e & 1))) & 0xffffu, hi = (c[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                *reinterpret_cast<unsigned*>(base + ulds[k] + e * KC * 2) = lo | (hi << 16);
            }
        }
        u32x4* Ws = reinterpret_cast<u32x4*>(base + XBYTES);
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            Ws[tid + i * 256] = wr[i];                                             // past WQ: padding nobody reads
        }
    };

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

    fetch(0);
    store(0);
    if (nchunks > 1) fetch(1);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        const uint4* Xs = reinterpret_cast<const uint4*>(smem_e + buf * BUF);
        const uint4* Ws = reinterpret_cast<const uint4*>(smem_e + buf * BUF + XBYTES);
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
        if (ch + 1 < nchunks) {
            store(buf ^ 1);                                                        // the buffer chunk ch-1 used: free since the last barrier
            if (ch + 2 < nchunks) fetch(ch + 2);                                   // in flight under chunk ch+1's MFMAs
        }
        __syncthreads();
    }

    // epilogue: lane = pixel l31 of the row, register i = output channel (i&3) + 8*(i>>2) + 4*half of the tile
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
            for (int i = 0; i < 16; ++i) store_out(dst + (size_t)(ct * 32 + (i & 3) + 8 * (i >> 2) + 4 * half) * HWo, acc[r][ct][i]);
    }
}

template <int KS, int S, int DL, int NT, int COT, class OutT>
int launch_enc(const u16* x, const u16* wp, OutT* y, int B, int Ci, int Co, int H, int W, int Ho, int Wo, void* stream) {
    constexpr int TH = 4 * NT;
    const int th = (Ho + TH - 1) / TH, tw = (Wo + TW - 1) / TW;
    const long long nb = (long long)B * th * tw;
    if (nb > 0x7fffffffLL || Co / (COT * 32) > 65535) return ECM_EUNSUP;
    constexpr int lds = enc_lds_bytes<KS, S, DL, NT, COT>();
    const bool vec = W % 8 == 0;
    const void* kern = vec ? reinterpret_cast<const void*>(conv2d_bf16<KS, S, DL, NT, COT, true, OutT>)
                           : reinterpret_cast<const void*>(conv2d_bf16<KS, S, DL, NT, COT, false, OutT>);
    const hipError_t e = ecm_allow_lds(kern, lds);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)nb, (unsigned)(Co / (COT * 32)));
    if (vec)
        hipLaunchKernelGGL((conv2d_bf16<KS, S, DL, NT, COT, true, OutT>), grid, dim3(256), lds, ecm_stream(stream), x, wp, y, Ci,
                           Co, H, W, Ho, Wo, th, tw);
    else
        hipLaunchKernelGGL((conv2d_bf16<KS, S, DL, NT, COT, false, OutT>), grid, dim3(256), lds, ecm_stream(stream), x, wp, y,
                           Ci, Co, H, W, Ho, Wo, th, tw);
    return ECM_LAUNCH_RESULT();
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

// ---- weight image: [Ci/16][k*k taps][Co][16 channels] bf16 from w [Co,Ci,k,k] -----------------------------------------------
__global__ void pack_bf16_2d(const float* __restrict__ w, u16* __restrict__ out, int Ci, int Co, int KK) {
    const long long n = (long long)Ci * KK * Co;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i & 15);
    long long r = i >> 4;
    const int co = (int)(r % Co); r /= Co;
    const int t = (int)(r % KK);
    const int ci = (int)(r / KK) * KC + j;
    out[i] = f2bf(w[((size_t)co * Ci + ci) * KK + t]);
}

}  // namespace

extern "C" long long ecm_conv2d_bf16_packed_elems(int Ci, int Co, int k) {
    return (Ci > 0 && Co > 0 && Ci % KC == 0 && (k == 1 || k == 3)) ? (long long)Ci * k * k * Co : 0;
}

extern "C" int ecm_conv2d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int k, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0 && (k == 1 || k == 3));
    if (Ci % KC != 0) return ECM_EUNSUP;
    const long long n = ecm_conv2d_bf16_packed_elems(Ci, Co, k);
    hipLaunchKernelGGL(pack_bf16_2d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ecm_stream(stream), w, packed, Ci, Co, k * k);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_conv2d_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, void* y, int B, int Ci, int Co,
                                   int H, int W, int k, int stride, int dil, int out_f32, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && H > 0 && W > 0 && (k == 1 || k == 3)
                  && (stride == 1 || stride == 2) && dil >= 1);
    if (Ci % KC != 0 || Co % 32 != 0) return ECM_EUNSUP;
    // element offsets inside one sample's planes stay 32-bit
    const long long Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long long)Ci * H * W >= 0x7fffffffLL || (long long)Co * Ho * Wo >= 0x7fffffffLL) return ECM_EUNSUP;
    if (out_f32) return dispatch<float>(x, wpacked, static_cast<float*>(y), B, Ci, Co, H, W, k, stride, dil, stream);
    return dispatch<u16>(x, wpacked, static_cast<u16*>(y), B, Ci, Co, H, W, k, stride, dil, stream);
}
