// Opt-in bf16 inference of the 3-D aggregation stack (ops.aggregation_dtype): forward-only kernels on bf16 NCDHW volumes
// with fp32 accumulation.  Reference layers: convbn_3d (cmfsm.py:49-58) and the hourglass's ConvTranspose3d (cmfsm.py:262-268).
//
// Convolution (k3 p1, stride 1|2) and transposed convolution (k3 s2 p1 op1) are the implicit-GEMM body of bf16_conv3d.h with
// bf16 storage as its operand policy: one term per operand, one product per k-step, all 28 slots staged from the weight image
// (its zero slot included), outputs rounded to bf16 once.
// No atomics: each output is one workgroup's fixed-order sum, so results are bit-reproducible.
// GroupNorm on bf16 volumes is gn3d.hip's two-stage forward (ecm_gn3d_stats_bf16 / ecm_gn3d_apply_bf16 / _f32_bf16).
#include "bf16_conv3d.h"

namespace {

struct Bf16Op {
    typedef u16 In;
    typedef u16 Out;
    typedef uint4 Held;                                            // a position's 8 channels, already the LDS vector
    static constexpr int NTERM = 1, CONV_SLOTS = 28, NPROD = 1;
    static constexpr int prod_w(int) { return 0; }
    static constexpr int prod_x(int) { return 0; }
    static constexpr int wg_per_cu(int) { return 2; }
    static __device__ __forceinline__ unsigned load(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
        return (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsrc, voff, soff, 0);
    }
    template <class Ld>
    static __device__ __forceinline__ void hold(Held& h, Ld ld) {
        unsigned v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = ld(c);
        h = pack8(v);
    }
    static __device__ __forceinline__ void terms(const Held& h, uint4 (&t)[NTERM]) { t[0] = h; }
    static __device__ __forceinline__ void wterms(float w, unsigned (&t)[NTERM]) { t[0] = f2bf(w); }
    static __device__ __forceinline__ Out out(float v) { return f2bf(v); }
};

// tile shapes: stride 1 and the transposed convolution 4 x 4 rows of 32 voxels; stride 2 2 x 4 (its halo is 2x wider)
constexpr int S1_TD = 4, S1_TH = 4, S2_TD = 2, S2_TH = 4, DC_TD = 4, DC_TH = 4;

bool conv_shape_ok(int Ci, int Co, long long D, long long H, long long W) {
    // 32-bit byte offsets inside one sample's volume
    return taps_channels_ok(Ci, Co) && (long long)Ci * D * H * W * 2 < 0x7fffffffLL;
}

}  // namespace

extern "C" long long ecm_conv3d_bf16_packed_elems(int Ci, int Co) { return taps_packed_elems<Bf16Op>(Ci, Co); }

extern "C" int ecm_conv3d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int transposed, void* stream) {
    ECM_CHECK_ARG(w && packed && Ci > 0 && Co > 0);
    if (Ci % 8 != 0) return ECM_EUNSUP;
    return launch_pack_taps<Bf16Op>(w, packed, Ci, Co, transposed, stream);
}

extern "C" int ecm_conv3d_k3_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, unsigned short* y, int B, int Ci,
                                      int Co, int D, int H, int W, int stride, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0);
    if (stride != 1 && stride != 2) return ECM_EUNSUP;
    if (!conv_shape_ok(Ci, Co, D, H, W)) return ECM_EUNSUP;
    const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if ((long long)Co * Do * Ho * Wo * 2 >= 0x7fffffffLL) return ECM_EUNSUP;
    if (stride == 1)
        return Co == 32 ? launch_conv3d_taps<Bf16Op, 1, 0, S1_TD, S1_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                        : launch_conv3d_taps<Bf16Op, 2, 0, S1_TD, S1_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
    return Co == 32 ? launch_conv3d_taps<Bf16Op, 1, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream)
                    : launch_conv3d_taps<Bf16Op, 2, 1, S2_TD, S2_TH>(x, wpacked, y, B, Ci, D, H, W, Do, Ho, Wo, stream);
}

extern "C" int ecm_deconv3d_k3s2_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, unsigned short* y, int B,
                                          int Ci, int Co, int D, int H, int W, void* stream) {
    ECM_CHECK_ARG(x && wpacked && y && B > 0 && Ci > 0 && Co > 0 && D > 0 && H > 0 && W > 0);
    if (!conv_shape_ok(Ci, Co, D, H, W) || (long long)Co * 8 * D * H * W * 2 >= 0x7fffffffLL) return ECM_EUNSUP;
    return Co == 32 ? launch_conv3d_taps<Bf16Op, 1, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, 2 * D, 2 * H, 2 * W, stream)
                    : launch_conv3d_taps<Bf16Op, 2, 2, DC_TD, DC_TH>(x, wpacked, y, B, Ci, D, H, W, 2 * D, 2 * H, 2 * W, stream);
}
