// The bf16 3-D implicit-GEMM body on v_mfma_f32_32x32x16_bf16, written once: conv3d_taps<Op, ...> is the k3 p1 convolution
// (stride 1|2) and the k3 s2 p1 transposed convolution of bf16_infer.hip (Op = bf16 storage) and of split_bf16.hip (Op = fp32
// split into three bf16 terms).  D[co][voxel] += sum_k A[co][k] * B[k][voxel].
//   k-step = 2 taps x 8 input channels: lane half h (= lane >> 5) takes tap slot 2s+h, element j its channel j, so that one
//   16-byte LDS read gives a lane one TERM of its fragment.  LDS holds the halo tile as [term][position][8 channels] and the
//   chunk's weight slice as [term][slot][co][8 channels].  An odd tap count is padded with a zero-weight slot whose activation
//   read is pointed at a zeroed LDS position (a zero weight times a staged Inf would be NaN); the slot's weight fragment comes
//   from the image, or is a constant where the family does not stage it (Op::CONV_SLOTS = 27).
//   Transposed convolution: output o = 2m + p per dimension takes tap k = 1 at input m (p = 0), or k = 0 at m+1 and k = 2 at m
//   (p = 1).  Each of the 8 output phases is a stride-1 convolution with 1..8 taps over the input grid; the phase is blockIdx.y
//   and every phase re-reads its small input tile through L2.  27 taps in all: every product is computed once.  An output extent
//   of 2n-1 (the data gradient of a stride-2 convolution on an odd extent) simply does not write the last odd plane.
// The operand policy Op carries what differs between the two families and nothing else:
//   In, load()          input element and its buffer load (bf16: the bits, zero-extended; fp32: the value)
//   Held, hold()        what a thread keeps per halo position while a chunk's loads are in flight; hold() fills it from a
//                       loader closure (channel -> loaded element), writing each element where it stays: staging the 8 values
//                       in an array first put every load of the fp32 family behind its own branch (+6 % instructions)
//   NTERM, terms()      bf16 terms per operand; Held -> the NTERM 16-byte LDS vectors of a position
//   wterms()            one fp32 weight -> its NTERM bf16 bit patterns (the pack kernel)
//   NPROD, prod_w/_x()  the products of a k-step as (weight term, activation term), in issue order
//   Out, out()          output element and the conversion of an accumulator to it
//   CONV_SLOTS          slots a convolution stages: 28, or 27 with the constant zero fragment
//   wg_per_cu(MODE)     __launch_bounds__' second argument
// Everything a thread carries across chunks lives in local arrays of ONE force-inlined function and is indexed by unrolled
// loops only, so it stays in VGPRs: no kernel built on this has a private segment.
#pragma once
#include "common.h"
#include "bf16.h"

namespace {

constexpr int TW = 32;          // output voxels along w per MFMA row (the B operand's 32 columns)
constexpr int NSLOT = 28;       // weight-image tap slots per 8-channel chunk and term: 27 taps + 1 zero (conv), or 8 phases padded to even

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

// MODE 0: conv stride 1, MODE 1: conv stride 2, MODE 2: transposed conv (phase PH); NSW_CONV: slots a convolution stages
template <int MODE, int PH, int TD, int TH, int NSW_CONV>
struct Geo {
    static constexpr int S = MODE == 1 ? 2 : 1;
    static constexpr int HALO = MODE == 2 ? 1 : 2;                 // extra input rows beyond S*(T-1)+1
    static constexpr int ID = S * (TD - 1) + 1 + HALO, IH = S * (TH - 1) + 1 + HALO, IW = S * (TW - 1) + 1 + HALO;
    static constexpr int NPOS = ID * IH * IW;
    static constexpr int ZERO = NPOS;                              // the zeroed position of the pad slot
    static constexpr int NTAPS = MODE == 2 ? dc_ntaps(PH) : 27;
    static constexpr int NS = MODE == 2 ? dc_nslots(PH) : NSLOT;   // slots this workgroup walks
    static constexpr int NSW = MODE == 2 ? NS : NSW_CONV;          // slots it stages
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

// 8 bf16 bit patterns (channels 0..7 of a position) -> the 16-byte LDS vector
__device__ __forceinline__ uint4 pack8(const unsigned (&t)[8]) {
    return make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
}

template <class Op, int CO_TILES, int MODE, int PH, int TD, int TH>
__device__ __forceinline__ void conv3d_taps_body(const typename Op::In* __restrict__ x, const u16* __restrict__ wp,
                                                 typename Op::Out* __restrict__ y, int Ci, int D, int H, int W, int Do, int Ho,
                                                 int Wo, int tiles_d, int tiles_h, int tiles_w, char* smem) {
    using G = Geo<MODE, PH, TD, TH, Op::CONV_SLOTS>;
    using In = typename Op::In;
    using Out = typename Op::Out;
    constexpr int S = G::S, IH = G::IH, IW = G::IW, NPOS = G::NPOS, NS = G::NS, NSW = G::NSW, NTERM = Op::NTERM;
    constexpr int COP = CO_TILES * 32;
    constexpr int ROWS = TD * TH, NT = ROWS / 4;
    static_assert(ROWS % 4 == 0, "rows split over 4 waves");
    constexpr int XT = NPOS + 1;                                   // positions per term, the zero position included
    constexpr int WT = NSW * COP;                                  // weight vectors per term
    uint4* Xs = reinterpret_cast<uint4*>(smem);                    // [NTERM][NPOS + 1][8 ch]
    uint4* Ws = Xs + NTERM * XT;                                   // [NTERM][NSW][COP][8 ch]

    int bid = ecm_xcd_tile(blockIdx.x, gridDim.x);
    const int td = bid % tiles_d; bid /= tiles_d;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int b = bid / tiles_h;
    const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;         // tile origin (input grid m for MODE 2)
    const int id0 = S * od0 + G::OFF0, ih0 = S * oh0 + G::OFF0, iw0 = S * ow0 + G::OFF0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;

    // staging: thread owns PP halo positions, loads their 8 channels of a chunk (one element per load, coalesced along w)
    constexpr int PP = (NPOS + 255) / 256;
    constexpr int NWQ = (WT + 255) / 256;                          // 16-byte weight vectors per thread and term
    const size_t HWi = (size_t)H * W, DHWi = (size_t)D * HWi;
    const In* xb = x + (size_t)b * Ci * DHWi;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<In*>(xb), 0, 0xffffffffu, 0x00020000);
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
        posoff[j] = ok ? (unsigned)((gz * HWi + gy * (size_t)W + gx) * sizeof(In)) : 0xffffffffu;
    }
    typename Op::Held xr[PP];                                      // the next chunk's values, in flight under the MFMAs
    auto fetch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            // channel plane c0+c (wave-uniform offset); positions outside the volume are zero padding, not loaded
            Op::hold(xr[j], [&](int c) __attribute__((always_inline)) {
                const unsigned soff = (unsigned)((size_t)(c0 + c) * DHWi * sizeof(In));
                return posoff[j] == 0xffffffffu ? 0 : Op::load(rsrc, posoff[j], soff);
            });
        }
    };
    // the chunk's weight slice (L2-resident: every workgroup reads the same few KB) goes straight to LDS
    auto store = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
            const uint4* wsrc = reinterpret_cast<const uint4*>(wp) + (((size_t)(c0 >> 3) * NTERM + t) * NSLOT + G::SLOT0) * COP;
#pragma unroll
            for (int i = 0; i < NWQ; ++i) {
                const int e = tid + i * 256;
                if (e < WT) Ws[t * WT + e] = wsrc[e];
            }
        }
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            const int p = tid + j * 256;
            uint4 xt[NTERM];
            Op::terms(xr[j], xt);
            if (p < NPOS) {
#pragma unroll
                for (int t = 0; t < NTERM; ++t) Xs[t * XT + p] = xt[t];
            }
        }
    };
    if (tid < NTERM) Xs[tid * XT + G::ZERO] = make_uint4(0, 0, 0, 0);

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
            const bool staged = 2 * s + 1 < NSW || slot < NSW;     // compile-time true except for the last step of CONV_SLOTS = 27
            const int wslot = staged ? slot : 0;
            bf16x8 a[NTERM][CO_TILES];
#pragma unroll
            for (int t = 0; t < NTERM; ++t)
#pragma unroll
                for (int ct = 0; ct < CO_TILES; ++ct) {
                    uint4 v = Ws[t * WT + wslot * COP + ct * 32 + l31];
                    if (!staged) v = make_uint4(0, 0, 0, 0);       // the pad slot's weight fragment
                    a[t][ct] = __builtin_bit_cast(bf16x8, v);
                }
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                const int pos = off < 0 ? G::ZERO : rbase[r] + off;
                bf16x8 bv[NTERM];
#pragma unroll
                for (int t = 0; t < NTERM; ++t) bv[t] = __builtin_bit_cast(bf16x8, Xs[t * XT + pos]);
#pragma unroll
                for (int q = 0; q < Op::NPROD; ++q)
#pragma unroll
                    for (int ct = 0; ct < CO_TILES; ++ct)
                        acc[r][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[Op::prod_w(q)][ct], bv[Op::prod_x(q)], acc[r][ct], 0, 0, 0);
            }
        }
    }

    // epilogue: lane = voxel l31 of the row, register i = output channel (i&3) + 8*(i>>2) + 4*half of the tile
    const size_t HWo = (size_t)Ho * Wo, DHWo = (size_t)Do * HWo;
    Out* yb = y + (size_t)b * COP * DHWo;
    constexpr int OS = MODE == 2 ? 2 : 1;
    constexpr int PD = MODE == 2 ? (PH >> 2) & 1 : 0, PHh = MODE == 2 ? (PH >> 1) & 1 : 0, PW = MODE == 2 ? PH & 1 : 0;
    const int mw = ow0 + l31;
    const int ow = OS * mw + PW;
    const bool okw = ow < Wo && (MODE != 2 || mw < W);
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        const int R = wave * NT + r;
        const int md = od0 + R / TH, mh = oh0 + R % TH;
        const int od = OS * md + PD, oh = OS * mh + PHh;
        const bool ok = okw && od < Do && oh < Ho && (MODE != 2 || (md < D && mh < H));
        if (!ok) continue;
        Out* dst = yb + (size_t)od * HWo + (size_t)oh * Wo + ow;
#pragma unroll
        for (int ct = 0; ct < CO_TILES; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = ct * 32 + mfma32_row(i, half);
                dst[(size_t)co * DHWo] = Op::out(acc[r][ct][i]);
            }
    }
}

// LDS: NTERM terms of (halo positions + the zero position) and of the staged weight slots
template <class Op, int MODE, int PH, int TD, int TH>
constexpr int conv3d_taps_lds_bytes(int co_tiles) {
    using G = Geo<MODE, PH, TD, TH, Op::CONV_SLOTS>;
    return Op::NTERM * (G::NPOS + 1 + G::NSW * co_tiles * 32) * 16;
}

template <class Op, int CO_TILES, int MODE, int TD, int TH>
__global__ __launch_bounds__(256, Op::wg_per_cu(MODE)) void conv3d_taps(const typename Op::In* __restrict__ x,
                                                                        const u16* __restrict__ wp, typename Op::Out* __restrict__ y,
                                                                        int Ci, int D, int H, int W, int Do, int Ho, int Wo,
                                                                        int tiles_d, int tiles_h, int tiles_w) {
    extern __shared__ __attribute__((aligned(16))) char smem_t[];
    if constexpr (MODE != 2) {
        conv3d_taps_body<Op, CO_TILES, MODE, 0, TD, TH>(x, wp, y, Ci, D, H, W, Do, Ho, Wo, tiles_d, tiles_h, tiles_w, smem_t);
    } else {
        switch (blockIdx.y) {
#define ECM_DC_PHASE(p) case p: conv3d_taps_body<Op, CO_TILES, 2, p, TD, TH>(x, wp, y, Ci, D, H, W, Do, Ho, Wo, tiles_d, tiles_h, tiles_w, smem_t); break;
            ECM_DC_PHASE(0) ECM_DC_PHASE(1) ECM_DC_PHASE(2) ECM_DC_PHASE(3)
            ECM_DC_PHASE(4) ECM_DC_PHASE(5) ECM_DC_PHASE(6) ECM_DC_PHASE(7)
#undef ECM_DC_PHASE
            default: break;
        }
    }
}

template <class Op, int CO_TILES, int MODE, int TD, int TH>
int launch_conv3d_taps(const typename Op::In* x, const u16* wp, typename Op::Out* y, int B, int Ci, int D, int H, int W, int Do,
                       int Ho, int Wo, void* stream) {
    // MODE 2 tiles the INPUT grid (one output voxel per phase per input voxel)
    const int gd = MODE == 2 ? D : Do, gh = MODE == 2 ? H : Ho, gw = MODE == 2 ? W : Wo;
    const int td = (gd + TD - 1) / TD, th = (gh + TH - 1) / TH, tw = (gw + TW - 1) / TW;
    const long long nb = (long long)B * td * th * tw;
    if (nb > 0x7fffffffLL) return ECM_EUNSUP;
    // MODE 2: every phase stages the same tile and phase 7 has the most slots
    const int lds = conv3d_taps_lds_bytes<Op, MODE, MODE == 2 ? 7 : 0, TD, TH>(CO_TILES);
    const void* kern = reinterpret_cast<const void*>(conv3d_taps<Op, CO_TILES, MODE, TD, TH>);
    const hipError_t e = ecm_allow_lds(kern, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((conv3d_taps<Op, CO_TILES, MODE, TD, TH>), dim3((unsigned)nb, MODE == 2 ? 8 : 1), dim3(256), lds,
                       ecm_stream(stream), x, wp, y, Ci, D, H, W, Do, Ho, Wo, td, th, tw);
    return ECM_LAUNCH_RESULT();
}

// ---- weight images: [Ci/8][NTERM][28 slots][Co][8 channels] bf16 ---------------------------------------------------------
// conv (w [Co,Ci,3,3,3]): slot t = kd*9 + kh*3 + kw, slot 27 zero; transposed (w [Ci,Co,3,3,3]): phase p's taps at dc_base(p)
template <class Op>
__global__ void pack_taps(const float* __restrict__ w, u16* __restrict__ out, int Ci, int Co, int transposed) {
    const long long n = (long long)(Ci / 8) * NSLOT * Co * 8;      // per term
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i & 7);
    long long r = i >> 3;
    const int co = (int)(r % Co); r /= Co;
    const int slot = (int)(r % NSLOT);
    const int chunk = (int)(r / NSLOT);
    const int ci = chunk * 8 + j;
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
    unsigned t[Op::NTERM];
    Op::wterms(v, t);
#pragma unroll
    for (int q = 0; q < Op::NTERM; ++q)
        out[((((size_t)chunk * Op::NTERM + q) * NSLOT + slot) * Co + co) * 8 + j] = (u16)t[q];
}

template <class Op>
constexpr long long taps_packed_elems(int Ci, int Co) {
    return (Ci > 0 && Co > 0 && Ci % 8 == 0) ? (long long)(Ci / 8) * Op::NTERM * NSLOT * Co * 8 : 0;
}

template <class Op>
int launch_pack_taps(const float* w, u16* packed, int Ci, int Co, int transposed, void* stream) {
    const long long n = taps_packed_elems<Op>(Ci, Co) / Op::NTERM;
    hipLaunchKernelGGL(pack_taps<Op>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ecm_stream(stream), w, packed, Ci, Co, transposed);
    return ECM_LAUNCH_RESULT();
}

// channel chunks of 8, output channels in tiles of 32
constexpr bool taps_channels_ok(int Ci, int Co) { return (Ci == 32 || Ci == 64) && (Co == 32 || Co == 64); }

}  // namespace
