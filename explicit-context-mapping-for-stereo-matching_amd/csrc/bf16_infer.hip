// Opt-in bf16 inference of the 3-D aggregation stack (ops.aggregation_dtype): forward-only kernels on bf16 NCDHW volumes
// with fp32 accumulation.  Reference layers: convbn_3d (cmfsm.py:49-58) and the hourglass's ConvTranspose3d (cmfsm.py:262-268).
//
// Convolution (k3 p1, stride 1|2) and transposed convolution (k3 s2 p1 op1) share ONE implicit-GEMM body on
// v_mfma_f32_32x32x16_bf16:  D[co][voxel] += sum_k A[co][k] * B[k][voxel].
//   k-step = 2 taps x 8 input channels: lane half h (= lane >> 5) takes tap slot 2s+h, element j its channel j, so that
//   one 16-byte LDS read gives a lane its whole fragment -- the halo tile sits in LDS as [position][8 channels] and the
//   weight slice as [slot][co][8 channels].  An odd tap count is padded with a zero-weight slot whose activation read is
//   pointed at a zeroed LDS position (a zero weight times a staged Inf would be NaN).
//   Transposed convolution: output o = 2m + p per dimension takes tap k = 1 at input m (p = 0), or k = 0 at m+1 and k = 2
//   at m (p = 1).  Each of the 8 output phases is a stride-1 convolution with 1..8 taps over the input grid; the phase is
//   blockIdx.y and every phase re-reads its small input tile through L2.  27 taps in all: every product is computed once.
// No atomics: each output is one workgroup's fixed-order sum, so results are bit-reproducible.
// GroupNorm on bf16 volumes is gn3d.hip's two-stage forward (ecm_gn3d_stats_bf16 / ecm_gn3d_apply_bf16 / _f32_bf16).
#include "common.h"
#include "bf16.h"

namespace {

constexpr int TW = 32;          // output voxels along w per MFMA row (the B operand's 32 columns)
constexpr int NSLOT = 28;       // weight-image tap slots per 8-channel chunk: 27 taps + 1 zero (conv), or 8 phases padded to even

// deconv phase p = pd*4 + ph*2 + pw: taps along a dimension are {k=1 at e=0} (p=0) or {k=0 at e=1, k=2 at e=0} (p=1)
__host__ __device__ constexpr int dc_ntaps(int p) { return (1 + ((p >> 2) & 1)) * (1 + ((p >> 1) & 1)) * (1 + (p & 1)); }
__host__ __device__ constexpr int dc_nslots(int p) { return (dc_ntaps(p) + 1) & ~1; }
__host__ __device__ constexpr int dc_base(int p) { return p == 0 ? 0 : dc_base(p - 1) + dc_nslots(p - 1); }
static_assert(dc_base(7) + dc_nslots(7) == NSLOT, "the 8 phases fill the 28 slots");

// tap t of deconv phase p -> (kd,kh,kw) of the weight and (ed,eh,ew) input offsets
__host__ __device__ constexpr void dc_tap(int p, int t, int* k, int* e) {
    const int pd[3] = {(p >> 2) & 1, (p >> 1) & 1, p & 1};
    const int n[3] = {1 + pd[0], 1 + pd[1], 1 + pd[2]};
    int idx[3] = {t / (n[1] * n[2]), (t / n[2]) % n[1], t % n[2]};
    for (int d = 0; d < 3; ++d) {
        if (!pd[d]) { k[d] = 1; e[d] = 0; }
        else if (idx[d] == 0) { k[d] = 0; e[d] = 1; }
        else { k[d] = 2; e[d] = 0; }
    }
}

// MODE 0: conv stride 1, MODE 1: conv stride 2, MODE 2: transposed conv (phase PH)
template <int MODE, int PH, int TD, int TH>
struct Geo {
    static constexpr int S = MODE == 1 ? 2 : 1;
    static constexpr int HALO = MODE == 2 ? 1 : 2;                 // extra input rows beyond S*(T-1)+1
    static constexpr int ID = S * (TD - 1) + 1 + HALO, IH = S * (TH - 1) + 1 + HALO, IW = S * (TW - 1) + 1 + HALO;
    static constexpr int NPOS = ID * IH * IW;
    static constexpr int ZERO = NPOS;                              // the zeroed position of the pad slot
    static constexpr int NTAPS = MODE == 2 ? dc_ntaps(PH) : 27;
    static constexpr int NS = MODE == 2 ? dc_nslots(PH) : NSLOT;   // slots this workgroup stages
    static constexpr int SLOT0 = MODE == 2 ? dc_base(PH) : 0;
    static constexpr int OFF0 = MODE == 2 ? 0 : -1;                // halo origin = S * tile origin + OFF0
    // LDS position offset of tap t (relative to the row/voxel base); -1 = pad slot
    static constexpr int tap_off(int t) {
        if (t >= NTAPS) return -1;
        int kd = t / 9, kh = (t / 3) % 3, kw = t % 3;
        if (MODE == 2) { int k[3] = {0, 0, 0}, e[3] = {0, 0, 0}; dc_tap(PH, t, k, e); kd = e[0]; kh = e[1]; kw = e[2]; }
        return (kd * IH + kh) * IW + kw;
    }
};

template <int CO_TILES, int MODE, int PH, int TD, int TH>
__device__ __forceinline__ void conv_bf16_body(const u16* __restrict__ x, const u16* __restrict__ wp, u16* __restrict__ y,
                                               int Ci, int D, int H, int W, int Do, int Ho, int Wo, int tiles_d, int tiles_h,
                                               int tiles_w, char* smem) {
    using G = Geo<MODE, PH, TD, TH>;
    constexpr int S = G::S, IH = G::IH, IW = G::IW, NPOS = G::NPOS, NS = G::NS;
    constexpr int COP = CO_TILES * 32;
    constexpr int ROWS = TD * TH, NT = ROWS / 4;
    static_assert(ROWS % 4 == 0, "rows split over 4 waves");
    uint4* Xs = reinterpret_cast<uint4*>(smem);                    // [NPOS + 1][8 ch]
    uint4* Ws = Xs + NPOS + 1;                                     // [NS][COP][8 ch]

    int bid = ecm_xcd_tile(blockIdx.x, gridDim.x);
    const int td = bid % tiles_d; bid /= tiles_d;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int b = bid / tiles_h;
    const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;         // tile origin (input grid m for MODE 2)
    const int id0 = S * od0 + G::OFF0, ih0 = S * oh0 + G::OFF0, iw0 = S * ow0 + G::OFF0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;

    // staging: thread owns PP halo positions, loads their 8 channels of a chunk (2-byte loads, coalesced along w)
    constexpr int PP = (NPOS + 255) / 256;
    constexpr int NWQ = (NS * COP + 255) / 256;                    // 16-byte weight vectors per thread
    const size_t HWi = (size_t)H * W, DHWi = (size_t)D * HWi;
    const u16* xb = x + (size_t)b * Ci * DHWi;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(xb), 0, 0xffffffffu, 0x00020000);
    unsigned posoff[PP];
#pragma unroll
    for (int j = 0; j < PP; ++j) {
        const int p = tid + j * 256;
        int t = p;
        const int xx = t % IW; t /= IW;
        const int hy = t % IH;
        const int dz = t / IH;
        const int gz = id0 + dz, gy = ih0 + hy, gx = iw0 + xx;
        const bool ok = p < NPOS && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        posoff[j] = ok ? (unsigned)((gz * HWi + gy * (size_t)W + gx) * 2) : 0xffffffffu;
    }
    uint4 xr[PP];
    auto fetch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            unsigned v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                // channel plane c0+c (wave-uniform offset); positions outside the volume are zero padding, not loaded
                const unsigned soff = (unsigned)((size_t)(c0 + c) * DHWi * 2);
                v[c] = posoff[j] == 0xffffffffu ? 0u : (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsrc, posoff[j], soff, 0);
            }
            xr[j] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
        }
    };
    // the chunk's weight slice (L2-resident: every workgroup reads the same few KB) goes straight to LDS
    auto store = [&](int c0) __attribute__((always_inline)) {
        const uint4* wsrc = reinterpret_cast<const uint4*>(wp) + ((size_t)(c0 >> 3) * NSLOT + G::SLOT0) * COP;
#pragma unroll
        for (int i = 0; i < NWQ; ++i) {
            const int e = tid + i * 256;
            if (e < NS * COP) Ws[e] = wsrc[e];
        }
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            const int p = tid + j * 256;
            if (p < NPOS) Xs[p] = xr[j];
        }
    };
    if (tid == 0) Xs[G::ZERO] = make_uint4(0, 0, 0, 0);

    f32x16 acc[NT][CO_TILES];
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
        for (int ct = 0; ct < CO_TILES; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[r][ct][i] = 0.f;
    int rbase[NT];
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        const int R = wave * NT + r, dz = R / TH, hy = R % TH;
        rbase[r] = ((S * dz) * IH + S * hy) * IW + S * l31;
    }

    fetch(0);
    for (int c0 = 0; c0 < Ci; c0 += 8) {
        if (c0) __syncthreads();                                   // previous chunk's LDS reads are done
        store(c0);
        __syncthreads();
        if (c0 + 8 < Ci) fetch(c0 + 8);                            // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < NS / 2; ++s) {
            const int slot = 2 * s + half;
            const int off0 = G::tap_off(2 * s), off1 = G::tap_off(2 * s + 1);
            const int off = half ? off1 : off0;
            bf16x8 a[CO_TILES];
#pragma unroll
            for (int ct = 0; ct < CO_TILES; ++ct) a[ct] = __builtin_bit_cast(bf16x8, Ws[slot * COP + ct * 32 + l31]);
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                const int pos = off < 0 ? G::ZERO : rbase[r] + off;
                const bf16x8 bv = __builtin_bit_cast(bf16x8, Xs[pos]);
#pragma unroll
                for (int ct = 0; ct < CO_TILES; ++ct)
                    acc[r][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ct], bv, acc[r][ct], 0, 0, 0);
            }
        }
    }

    // epilogue: lane = voxel l31 of the row, register i = output channel (i&3) + 8*(i>>2) + 4*half of the tile
    const size_t HWo = (size_t)Ho * Wo, DHWo = (size_t)Do * HWo;
    u16* yb = y + (size_t)b * COP * DHWo;
    constexpr int OS = MODE == 2 ? 2 : 1;
    constexpr int PD = MODE == 2 ? (PH >> 2) & 1 : 0, PHh = MODE == 2 ? (PH >> 1) & 1 : 0, PW = MODE == 2 ? PH & 1 : 0;
    const int mw = ow0 + l31;
    const int ow = OS * mw + PW;
    const bool okw = MODE == 2 ? mw < W : ow < Wo;
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        const int R = wave * NT + r;
        const int md = od0 + R / TH, mh = oh0 + R % TH;
        const int od = OS * md + PD, oh = OS * mh + PHh;
        const bool ok = okw && (MODE == 2 ? (md < D && mh < H) : (od < Do && oh < Ho));
        if (!ok) continue;
        u16* dst = yb + (size_t)od * HWo + (size_t)oh * Wo + ow;
#pragma unroll
        for (int ct = 0; ct < CO_TILES; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = ct * 32 + mfma32_row(i, half);
                dst[(size_t)co * DHWo] = f2bf(acc[r][ct][i]);
            }
    }
}

// LDS: halo positions + the zero position + the weight slots
template <int MODE, int PH, int TD, int TH>
constexpr int conv_lds_bytes(int co_tiles) {
    return (Geo<MODE, PH, TD, TH>::NPOS + 1 + Geo<MODE, PH, TD, TH>::NS * co_tiles * 32) * 16;
}

template <int CO_TILES, int MODE, int TD, int TH>
__global__ __launch_bounds__(256, 2) void conv3d_bf16(const u16* __restrict__ x, const u16* __restrict__ wp, u16* __restrict__ y,
                                                      int Ci, int D, int H, int W, int Do, int Ho, int Wo, int tiles_d,
                                                      int tiles_h, int tiles_w) {
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    if constexpr (MODE != 2) {
        conv_bf16_body<CO_TILES, MODE, 0, TD, TH>(x, wp, y, Ci, D, H, W, Do, Ho, Wo, tiles_d, tiles_h, tiles_w, smem_c);
    } else {
        switch (blockIdx.y) {
#define ECM_DC_PHASE(p) case p: conv_bf16_body<CO_TILES, 2, p, TD, TH>(x, wp, y, Ci, D, H, W, Do, Ho, Wo, tiles_d, tiles_h, tiles_w, smem_c); break;
            ECM_DC_PHASE(0) ECM_DC_PHASE(1) ECM_DC_PHASE(2) ECM_DC_PHASE(3)
            ECM_DC_PHASE(4) ECM_DC_PHASE(5) ECM_DC_PHASE(6) ECM_DC_PHASE(7)
#undef ECM_DC_PHASE
            default: break;
        }
    }
}

// tile shapes: stride 1 and the transposed convolution 4 x 4 rows of 32 voxels; stride 2 2 x 4 (its halo is 2x wider)
constexpr int S1_TD = 4, S1_TH = 4, S2_TD = 2, S2_TH = 4, DC_TD = 4, DC_TH = 4;

template <int CO_TILES, int MODE, int TD, int TH>
int launch_conv_bf16(const u16* x, const u16* wp, u16* y, int B, int Ci, int D, int H, int W, int Do, int Ho, int Wo,
                     void* stream) {
    // MODE 2 tiles the INPUT grid (one output voxel per phase per input voxel)
    const int gd = MODE == 2 ? D : Do, gh = MODE == 2 ? H : Ho, gw = MODE == 2 ? W : Wo;
    const int td = (gd + TD - 1) / TD, th = (gh + TH - 1) / TH, tw = (gw + TW - 1) / TW;
    const long long nb = (long long)B * td * th * tw;
    if (nb > 0x7fffffffLL) return ECM_EUNSUP;
    // the largest phase's halo (MODE 2: every phase stages the same tile; slots differ)
    const int lds = conv_lds_bytes<MODE, MODE == 2 ? 7 : 0, TD, TH>(CO_TILES);     // phase 7 has the most slots
    const void* kern = reinterpret_cast<const void*>(conv3d_bf16<CO_TILES, MODE, TD, TH>);
    const hipError_t e = ecm_allow_lds(kern, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((conv3d_bf16<CO_TILES, MODE, TD, TH>), dim3((unsigned)nb, MODE == 2 ? 8 : 1), dim3(256), lds,
                       ecm_stream(stream), x, wp, y, Ci, D, H, W, Do, Ho, Wo, td, th, tw);
    return ECM_LAUNCH_RESULT();
}

// ---- weight images: [Ci/8][28 slots][Co][8 channels] bf16 -----------------------------------------------------------------
// conv (w [Co,Ci,3,3,3]): slot t = kd*9 + kh*3 + kw, slot 27 zero; transposed (w [Ci,Co,3,3,3]): phase p's taps at dc_base(p)
__global__ void pack_bf16(const float* __restrict__ w, u16* __restrict__ out, int Ci, int Co, int transposed) {
    const long long n = (long long)(Ci / 8) * NSLOT * Co * 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i & 7);
    long long r = i >> 3;
    const int co = (int)(r % Co); r /= Co;
    const int slot = (int)(r % NSLOT);
    const int ci = (int)(r / NSLOT) * 8 + j;
    float v = 0.f;
    if (!transposed) {
        if (slot < 27) v = w[((size_t)co * Ci + ci) * 27 + slot];
    } else {
        int p = 0;
        while (p < 7 && slot >= dc_base(p + 1)) ++p;
        const int t = slot - dc_base(p);
        if (t < dc_ntaps(p)) {
            int k[3] = {0, 0, 0}, e[3] = {0, 0, 0};
            dc_tap(p, t, k, e);
            v = w[((size_t)ci * Co + co) * 27 + (k[0] * 3 + k[1]) * 3 + k[2]];
        }
    }
    out[i] = f2bf(v);
}

bool conv_shape_ok(int Ci, int Co, long long D, long long H, long long W) {
    // channel chunks of 8, output channels in tiles of 32; 32-bit byte offsets inside one sample's volume
    return (Ci == 32 || Ci == 64) && (Co == 32 || Co == 64) && (long long)Ci * D * H * W * 2 < 0x7fffffffLL;
}

}  // namespace

extern "C" long long ecm_conv3d_bf16_packed_elems(int Ci, int Co) {
    return (Ci > 0 && Co > 0 && Ci % 8 == 0) ? (long long)(Ci / 8) * NSLOT * Co * 8 : 0;
}

extern "C" int ecm_conv3d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int transposed, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0);
    if (Ci % 8 != 0) return ECM_EUNSUP;
    const long long n = ecm_conv3d_bf16_packed_elems(Ci, Co);
    hipLaunchKernelGGL(pack_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ecm_stream(stream), w, packed, Ci, Co, transposed);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_conv3d_k3_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, unsigned short* y, int B, int Ci,
                                      int Co, int D, int H, int W, int stride, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2));
    if (!conv_shape_ok(Ci, Co, D, H, W)) return ECM_EUNSUP;
    const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long long)Co * Do * Ho * Wo * 2 >= 0x7fffffffLL) return ECM_EUNSUP;
    if (stride == 1)
        return Co == 32 ? launch_conv_bf16<1, 0, S1_TD, S1_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                        : launch_conv_bf16<2, 0, S1_TD, S1_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
    return Co == 32 ? launch_conv_bf16<1, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                    : launch_conv_bf16<2, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
}

extern "C" int ecm_deconv3d_k3s2_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, unsigned short* y, int B,
                                          int Ci, int Co, int D, int H, int W, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0);
    if (!conv_shape_ok(Ci, Co, D, H, W) || (long long)Co * 8 * D * H * W * 2 >= 0x7fffffffLL) return ECM_EUNSUP;
    return Co == 32 ? launch_conv_bf16<1, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, 2 * D, 2 * H, 2 * W, stream)
                    : launch_conv_bf16<2, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, 2 * D, 2 * H, 2 * W, stream);
}
