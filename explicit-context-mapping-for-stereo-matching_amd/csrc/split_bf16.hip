// Opt-in split-bf16 products (ops.split_products) for the stride-2 3-D convolutions: Conv3d k3 p1 s2 (the hourglass's
// conv1/conv3, cmfsm.py:244-258) and ConvTranspose3d k3 s2 p1 op1 (conv5/conv6, cmfsm.py:262-268), forward and -- as each
// other's adjoint -- data gradient.  fp32 NCDHW in, fp32 NCDHW out, fp32-equivalent results on the bf16 matrix cores.
//
// The split.  Every fp32 operand x becomes three bf16 terms, x = x1 + x2 + x3, by truncation (split3 below;
// tests/test_split_bf16_cpu.py restates the same bit operations in torch):
//     x1 = top 16 bits of x;  r1 = x - x1 (exact in fp32);  x2 = top 16 bits of r1;  r2 = r1 - x2 (exact);  x3 = top 16 bits of r2.
//   Truncation, not round-to-nearest: it never overflows (FLT_MAX keeps a finite x1), every remainder has the sign of x, and
//   each step strips 8 significand bits, so r2 has at most 8 and x3 holds it exactly.
//   Range: x1 + x2 + x3 == x exactly for every finite x whose lowest set bit is >= 2^-133 (the smallest bf16 subnormal) -- all
//   |x| >= 2^-110, and zero.  Below that the bits under 2^-133 are dropped (|x - (x1+x2+x3)| < 2^-133), and x3 (then x2) is a bf16
//   SUBNORMAL: fp32 equivalence is guaranteed for |x| >= 2^-110 only (measured on the MI355X, DESIGN.md section 14: the matrix
//   core does not flush a bf16-subnormal activation term, so below the range only those dropped bits are lost).
//   Non-finite x: (x, 0, 0) -- Inf stays Inf and multiplies the weight once (Inf - Inf would be NaN), NaN keeps a quiet bit.
//   (Inf times a non-zero weight that is exactly a bf16 value meets that weight's zero second term: NaN where fp32 gives Inf.)
// The products.  x*w ~= x1w1 + x1w2 + x2w1 + x1w3 + x3w1 + x2w2, the six leading cross products, each a
// v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator; the dropped x2w3, x3w2 (<= 2^-24 |xw| each) and x3w3 (2^-32) are below
// fp32's own rounding.
//
// The kernel is bf16_infer.hip's implicit GEMM  D[co][voxel] += sum_k A[co][k] * B[k][voxel]:
//   k-step = 2 taps x 8 input channels: lane half h (= lane >> 5) takes tap slot 2s+h, element j its channel j; one 16-byte
//   LDS read gives a lane one TERM of its fragment.  LDS holds the halo tile as [term][position][8 channels] and the chunk's
//   weight slice as [term][slot][co][8 channels]; fp32 is loaded, split once as it is staged, and never split again.
//   An odd tap count is padded with a slot whose weight fragment is zero and whose activation read points at a zeroed LDS
//   position (a zero weight times a staged Inf would be NaN).
//   Transposed convolution: output o = 2m + p per dimension takes tap k = 1 at input m (p = 0), or k = 0 at m+1 and k = 2 at m
//   (p = 1); each of the 8 output phases (blockIdx.y) is a stride-1 convolution with 1..8 taps over the input grid.  The output
//   extent per dimension is 2n or 2n-1 (the data gradient of a stride-2 convolution on an odd extent): the last odd plane is
//   simply not written.
// LDS budget (160 KiB per CU).  Stride 2: a 2 x 2 x 32 output tile has a 5 x 5 x 65 halo = 1625 positions x 48 B (three terms)
//   = 76 KB, and 27 slots x 64 co x 48 B = 81 KB of weights: 157 KB, one workgroup per CU (the zero slot is not staged: its
//   fragment is a constant).  Transposed: a 4 x 4 x 32 input tile, 5 x 5 x 33 halo = 39 KB + at most 8 slots = 24 KB: two per CU.
// No atomics: each output is one workgroup's fixed-order sum, so results are bit-reproducible.
#include "common.h"
#include "bf16.h"

namespace {

constexpr int TW = 32;          // output voxels along w per MFMA row (the B operand's 32 columns)
constexpr int NSLOT = 28;       // weight-image tap slots per 8-channel chunk and term: 27 taps + 1 zero (conv), or 8 phases padded to even
constexpr int NTERM = 3;        // bf16 terms per fp32 operand
constexpr int CONV_SLOTS = 27;  // slots the convolution stages (slot 27 is the constant zero fragment)

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

// x -> the bf16 bit patterns of its three terms (see the header comment)
__device__ __forceinline__ void split3(float x, unsigned& t1, unsigned& t2, unsigned& t3) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const bool fin = (u & 0x7f800000u) != 0x7f800000u;
    const bool nan = !fin && (u & 0x007fffffu) != 0u;
    const float r1 = x - __builtin_bit_cast(float, u & 0xffff0000u);
    const unsigned v1 = __builtin_bit_cast(unsigned, r1);
    const float r2 = r1 - __builtin_bit_cast(float, v1 & 0xffff0000u);
    const unsigned v2 = __builtin_bit_cast(unsigned, r2);
    t1 = (u >> 16) | (nan ? 0x40u : 0u);
    t2 = fin ? v1 >> 16 : 0u;
    t3 = fin ? v2 >> 16 : 0u;
}

// MODE 1: conv stride 2, MODE 2: transposed conv (phase PH)
template <int MODE, int PH, int TD, int TH>
struct Geo {
    static constexpr int S = MODE == 1 ? 2 : 1;
    static constexpr int HALO = MODE == 2 ? 1 : 2;                 // extra input rows beyond S*(T-1)+1
    static constexpr int ID = S * (TD - 1) + 1 + HALO, IH = S * (TH - 1) + 1 + HALO, IW = S * (TW - 1) + 1 + HALO;
    static constexpr int NPOS = ID * IH * IW;
    static constexpr int ZERO = NPOS;                              // the zeroed position of the pad slot
    static constexpr int NTAPS = MODE == 2 ? dc_ntaps(PH) : 27;
    static constexpr int NS = MODE == 2 ? dc_nslots(PH) : NSLOT;   // slots this workgroup walks
    static constexpr int NSW = MODE == 2 ? NS : CONV_SLOTS;        // slots it stages
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
__device__ __forceinline__ void conv_split_body(const float* __restrict__ x, const u16* __restrict__ wp, float* __restrict__ y,
                                                int Ci, int D, int H, int W, int Do, int Ho, int Wo, int tiles_d, int tiles_h,
                                                int tiles_w, char* smem) {
    using G = Geo<MODE, PH, TD, TH>;
    constexpr int S = G::S, IH = G::IH, IW = G::IW, NPOS = G::NPOS, NS = G::NS, NSW = G::NSW;
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

    // staging: thread owns PP halo positions, loads their 8 channels of a chunk as fp32 (coalesced along w)
    constexpr int PP = (NPOS + 255) / 256;
    constexpr int NWQ = (WT + 255) / 256;                          // 16-byte weight vectors per thread and term
    const size_t HWi = (size_t)H * W, DHWi = (size_t)D * HWi;
    const float* xb = x + (size_t)b * Ci * DHWi;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, 0xffffffffu, 0x00020000);
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
        posoff[j] = ok ? (unsigned)((gz * HWi + gy * (size_t)W + gx) * 4) : 0xffffffffu;
    }
    float xr[PP][8];                                               // the next chunk's fp32 values, in flight under the MFMAs
    auto fetch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < PP; ++j)
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                // channel plane c0+c (wave-uniform offset); positions outside the volume are zero padding, not loaded
                const unsigned soff = (unsigned)((size_t)(c0 + c) * DHWi * 4);
                xr[j][c] = posoff[j] == 0xffffffffu
                               ? 0.f
                               : __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rsrc, posoff[j], soff, 0));
            }
    };
    // the chunk's weight slice (already split by the pack kernel; L2-resident) goes straight to LDS, the activations are split here
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
            unsigned t1[8], t2[8], t3[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) split3(xr[j][c], t1[c], t2[c], t3[c]);
            if (p < NPOS) {
                Xs[p] = make_uint4(t1[0] | (t1[1] << 16), t1[2] | (t1[3] << 16), t1[4] | (t1[5] << 16), t1[6] | (t1[7] << 16));
                Xs[XT + p] = make_uint4(t2[0] | (t2[1] << 16), t2[2] | (t2[3] << 16), t2[4] | (t2[5] << 16), t2[6] | (t2[7] << 16));
                Xs[2 * XT + p] = make_uint4(t3[0] | (t3[1] << 16), t3[2] | (t3[3] << 16), t3[4] | (t3[5] << 16), t3[6] | (t3[7] << 16));
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
            const bool staged = 2 * s + 1 < NSW || slot < NSW;     // compile-time true except for the conv's last step
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
                // the six leading cross products (weight term, activation term), smallest first
                constexpr int PW_[6] = {2, 0, 1, 1, 0, 0}, PX_[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int q = 0; q < 6; ++q)
#pragma unroll
                    for (int ct = 0; ct < CO_TILES; ++ct)
                        acc[r][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PW_[q]][ct], bv[PX_[q]], acc[r][ct], 0, 0, 0);
            }
        }
    }

    // epilogue: lane = voxel l31 of the row, register i = output channel (i&3) + 8*(i>>2) + 4*half of the tile
    const size_t HWo = (size_t)Ho * Wo, DHWo = (size_t)Do * HWo;
    float* yb = y + (size_t)b * COP * DHWo;
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
        float* dst = yb + (size_t)od * HWo + (size_t)oh * Wo + ow;
#pragma unroll
        for (int ct = 0; ct < CO_TILES; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = ct * 32 + mfma32_row(i, half);
                dst[(size_t)co * DHWo] = acc[r][ct][i];
            }
    }
}

// LDS: three terms of (halo positions + the zero position) and of the staged weight slots
template <int MODE, int PH, int TD, int TH>
constexpr int split_lds_bytes(int co_tiles) {
    return NTERM * (Geo<MODE, PH, TD, TH>::NPOS + 1 + Geo<MODE, PH, TD, TH>::NSW * co_tiles * 32) * 16;
}

// tile shapes: stride 2 2 x 2 rows of 32 voxels (one workgroup per CU), the transposed convolution 4 x 4 (two per CU)
constexpr int S2_TD = 2, S2_TH = 2, DC_TD = 4, DC_TH = 4;
constexpr int LDS_LIMIT = 160 * 1024;
static_assert(split_lds_bytes<1, 0, S2_TD, S2_TH>(2) <= LDS_LIMIT, "the stride-2 tile fits one CU's LDS");
static_assert(2 * split_lds_bytes<2, 7, DC_TD, DC_TH>(2) <= LDS_LIMIT, "two transposed-convolution workgroups fit one CU's LDS");

template <int CO_TILES, int MODE, int TD, int TH>
__global__ __launch_bounds__(256, MODE == 2 ? 2 : 1) void conv3d_split(const float* __restrict__ x, const u16* __restrict__ wp,
                                                                      float* __restrict__ y, int Ci, int D, int H, int W, int Do,
                                                                      int Ho, int Wo, int tiles_d, int tiles_h, int tiles_w) {
    extern __shared__ __attribute__((aligned(16))) char smem_s[];
    if constexpr (MODE != 2) {
        conv_split_body<CO_TILES, MODE, 0, TD, TH>(x, wp, y, Ci, D, H, W, Do, Ho, Wo, tiles_d, tiles_h, tiles_w, smem_s);
    } else {
        switch (blockIdx.y) {
#define ECM_DC_PHASE(p) case p: conv_split_body<CO_TILES, 2, p, TD, TH>(x, wp, y, Ci, D, H, W, Do, Ho, Wo, tiles_d, tiles_h, tiles_w, smem_s); break;
            ECM_DC_PHASE(0) ECM_DC_PHASE(1) ECM_DC_PHASE(2) ECM_DC_PHASE(3)
            ECM_DC_PHASE(4) ECM_DC_PHASE(5) ECM_DC_PHASE(6) ECM_DC_PHASE(7)
#undef ECM_DC_PHASE
            default: break;
        }
    }
}

template <int CO_TILES, int MODE, int TD, int TH>
int launch_conv_split(const float* x, const u16* wp, float* y, int B, int Ci, int D, int H, int W, int Do, int Ho, int Wo,
                      void* stream) {
    // MODE 2 tiles the INPUT grid (one output voxel per phase per input voxel)
    const int gd = MODE == 2 ? D : Do, gh = MODE == 2 ? H : Ho, gw = MODE == 2 ? W : Wo;
    const int td = (gd + TD - 1) / TD, th = (gh + TH - 1) / TH, tw = (gw + TW - 1) / TW;
    const long long nb = (long long)B * td * th * tw;
    if (nb > 0x7fffffffLL) return ECM_EUNSUP;
    const int lds = split_lds_bytes<MODE, MODE == 2 ? 7 : 0, TD, TH>(CO_TILES);      // phase 7 has the most slots
    const void* kern = reinterpret_cast<const void*>(conv3d_split<CO_TILES, MODE, TD, TH>);
    const hipError_t e = ecm_allow_lds(kern, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((conv3d_split<CO_TILES, MODE, TD, TH>), dim3((unsigned)nb, MODE == 2 ? 8 : 1), dim3(256), lds,
                       ecm_stream(stream), x, wp, y, Ci, D, H, W, Do, Ho, Wo, td, th, tw);
    return ECM_LAUNCH_RESULT();
}

// ---- weight images: [Ci/8][3 terms][28 slots][Co][8 channels] bf16 --------------------------------------------------------
// conv (w [Co,Ci,3,3,3]): slot t = kd*9 + kh*3 + kw, slot 27 zero; transposed (w [Ci,Co,3,3,3]): phase p's taps at dc_base(p)
__global__ void pack_split(const float* __restrict__ w, u16* __restrict__ out, int Ci, int Co, int transposed) {
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
    unsigned t[NTERM];
    split3(v, t[0], t[1], t[2]);
#pragma unroll
    for (int q = 0; q < NTERM; ++q)
        out[((((size_t)chunk * NTERM + q) * NSLOT + slot) * Co + co) * 8 + j] = (u16)t[q];
}

bool split_shape_ok(int Ci, int Co, long long nin, long long nout) {
    // channel chunks of 8, output channels in tiles of 32; 32-bit byte offsets inside one sample's volume
    return (Ci == 32 || Ci == 64) && (Co == 32 || Co == 64) && Ci * nin * 4 < 0x7fffffffLL && Co * nout * 4 < 0x7fffffffLL;
}

}  // namespace

extern "C" long long ecm_conv3d_split_packed_elems(int Ci, int Co) {
    return (Ci > 0 && Co > 0 && Ci % 8 == 0) ? (long long)(Ci / 8) * NTERM * NSLOT * Co * 8 : 0;
}

extern "C" int ecm_conv3d_split_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int transposed, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0);
    if (Ci % 8 != 0) return ECM_EUNSUP;
    const long long n = ecm_conv3d_split_packed_elems(Ci, Co) / NTERM;
    hipLaunchKernelGGL(pack_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ecm_stream(stream), w, packed, Ci, Co, transposed);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_conv3d_k3s2_split_fwd(const float* x, const unsigned short* wpacked, float* y, int B, int Ci, int Co, int D,
                                         int H, int W, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0);
    const int Do = (D - 1) / 2 + 1, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (!split_shape_ok(Ci, Co, (long long)D * H * W, (long long)Do * Ho * Wo)) return ECM_EUNSUP;
    return Co == 32 ? launch_conv_split<1, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                    : launch_conv_split<2, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
}

extern "C" int ecm_deconv3d_k3s2_split_fwd(const float* x, const unsigned short* wpacked, float* y, int B, int Ci, int Co, int D,
                                           int H, int W, int Do, int Ho, int Wo, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0);
    // output extent per dim is 2n (output_padding 1) or 2n-1 (dgrad of a stride-2 conv on an odd extent)
    if (Do > 2 * D || Do < 2 * D - 1 || Ho > 2 * H || Ho < 2 * H - 1 || Wo > 2 * W || Wo < 2 * W - 1) return ECM_EUNSUP;
    if (!split_shape_ok(Ci, Co, (long long)D * H * W, (long long)Do * Ho * Wo)) return ECM_EUNSUP;
    return Co == 32 ? launch_conv_split<1, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                    : launch_conv_split<2, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
}
