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
// The kernel is the implicit-GEMM body of bf16_conv3d.h with this split as its operand policy: fp32 is loaded, split once as it
// is staged (the weights by the pack kernel), and never split again; LDS holds three terms of the halo tile and of the chunk's
// weight slice.
// LDS budget (160 KiB per CU).  Stride 2: a 2 x 2 x 32 output tile has a 5 x 5 x 65 halo = 1625 positions x 48 B (three terms)
//   = 76 KB, and 27 slots x 64 co x 48 B = 81 KB of weights: 157 KB, one workgroup per CU (the zero slot is not staged: its
//   fragment is a constant).  Transposed: a 4 x 4 x 32 input tile, 5 x 5 x 33 halo = 39 KB + at most 8 slots = 24 KB: two per CU.
// No atomics: each output is one workgroup's fixed-order sum, so results are bit-reproducible.
#include "bf16_conv3d.h"

namespace {

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

struct SplitOp {
    typedef float In;
    typedef float Out;
    struct Held { float c[8]; };                                   // a position's 8 channels as loaded: split when staged
    // three bf16 terms per fp32 operand; the convolution stages 27 slots (slot 27 is the constant zero fragment)
    static constexpr int NTERM = 3, CONV_SLOTS = 27, NPROD = 6;
    // the six leading cross products (weight term, activation term), smallest first
    static constexpr int prod_w(int q) { constexpr int t[NPROD] = {2, 0, 1, 1, 0, 0}; return t[q]; }
    static constexpr int prod_x(int q) { constexpr int t[NPROD] = {0, 2, 1, 0, 1, 0}; return t[q]; }
    static constexpr int wg_per_cu(int mode) { return mode == 2 ? 2 : 1; }
    static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
        return __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0));
    }
    template <class Ld>
    static __device__ __forceinline__ void hold(Held& h, Ld ld) {
#pragma unroll
        for (int c = 0; c < 8; ++c) h.c[c] = ld(c);
    }
    static __device__ __forceinline__ void terms(const Held& h, uint4 (&t)[NTERM]) {
        unsigned s[NTERM][8];
#pragma unroll
        for (int c = 0; c < 8; ++c) split3(h.c[c], s[0][c], s[1][c], s[2][c]);
#pragma unroll
        for (int q = 0; q < NTERM; ++q) t[q] = pack8(s[q]);
    }
    static __device__ __forceinline__ void wterms(float w, unsigned (&t)[NTERM]) { split3(w, t[0], t[1], t[2]); }
    static __device__ __forceinline__ Out out(float v) { return v; }
};

// tile shapes: stride 2 2 x 2 rows of 32 voxels (one workgroup per CU), the transposed convolution 4 x 4 (two per CU)
constexpr int S2_TD = 2, S2_TH = 2, DC_TD = 4, DC_TH = 4;
constexpr int LDS_LIMIT = 160 * 1024;
static_assert(conv3d_taps_lds_bytes<SplitOp, 1, 0, S2_TD, S2_TH>(2) <= LDS_LIMIT, "the stride-2 tile fits one CU's LDS");
static_assert(2 * conv3d_taps_lds_bytes<SplitOp, 2, 7, DC_TD, DC_TH>(2) <= LDS_LIMIT,
              "two transposed-convolution workgroups fit one CU's LDS");

bool split_shape_ok(int Ci, int Co, long long nin, long long nout) {
    // 32-bit byte offsets inside one sample's volume
    return taps_channels_ok(Ci, Co) && Ci * nin * 4 < 0x7fffffffLL && Co * nout * 4 < 0x7fffffffLL;
}

}  // namespace

extern "C" long long ecm_conv3d_split_packed_elems(int Ci, int Co) { return taps_packed_elems<SplitOp>(Ci, Co); }

extern "C" int ecm_conv3d_split_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int transposed, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0);
    if (Ci % 8 != 0) return ECM_EUNSUP;
    return launch_pack_taps<SplitOp>(w, packed, Ci, Co, transposed, stream);
}

extern "C" int ecm_conv3d_k3s2_split_fwd(const float* x, const unsigned short* wpacked, float* y, int B, int Ci, int Co, int D,
                                         int H, int W, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0);
    const int Do = (D - 1) / 2 + 1, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (!split_shape_ok(Ci, Co, (long long)D * H * W, (long long)Do * Ho * Wo)) return ECM_EUNSUP;
    return Co == 32 ? launch_conv3d_taps<SplitOp, 1, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                    : launch_conv3d_taps<SplitOp, 2, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
}

extern "C" int ecm_deconv3d_k3s2_split_fwd(const float* x, const unsigned short* wpacked, float* y, int B, int Ci, int Co, int D,
                                           int H, int W, int Do, int Ho, int Wo, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0 && Do > 0 && Ho > 0 && Wo > 0);
    // output extent per dim is 2n (output_padding 1) or 2n-1 (dgrad of a stride-2 conv on an odd extent)
    if (Do > 2 * D || Do < 2 * D - 1 || Ho > 2 * H || Ho < 2 * H - 1 || Wo > 2 * W || Wo < 2 * W - 1) return ECM_EUNSUP;
    if (!split_shape_ok(Ci, Co, (long long)D * H * W, (long long)Do * Ho * Wo)) return ECM_EUNSUP;
    return Co == 32 ? launch_conv3d_taps<SplitOp, 1, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                    : launch_conv3d_taps<SplitOp, 2, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
}
