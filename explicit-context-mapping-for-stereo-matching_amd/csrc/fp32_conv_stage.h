// The operand staging of the fp32 implicit-GEMM kernels on v_mfma_f32_32x32x2_f32, written once: conv3d_k3_mfma (conv3d.hip),
// deconv3d_k3s2_mfma (deconv3d.hip) and conv2d_mfma (conv2d_kernel.h) are this pipeline around their own tap block and epilogue.
//   GEMM view:  D[co][voxel] += sum_k A[co][k] * B[k][voxel],  k = (tap, ci), walked in chunks of CIC input channels.
//   A = weights    : lane l holds W[co = l&31][k = l>>5], read from the chunk's LDS slice [tap][CIC][COP] (conflict-free).  The
//        slice comes straight from the packed image [tap][channels][COP] by global_load_lds_dwordx4 (no VGPRs; lands at wave
//        base + lane*16) into a double-buffered area: chunk c+1's slice is in flight under chunk c's MFMAs.
//   B = activations: lane l holds X[k = l>>5][voxel = l&31] -- 32 consecutive x of one row of the staged halo tile
//        [CIC][ID][IH][IW]; NC(D)HW as it stands is the operand layout, no transposition anywhere.
//   Halo staging is software-pipelined through registers: a thread owns PP fixed positions of the halo window (offsets and
//   bounds computed once per tile) and walks the CIC channel planes of a chunk.  The loads of chunk c+1 are issued under the
//   MFMAs of chunk c and only waited for when they are written to LDS.  They go through buffer descriptors (one per channel
//   plane, built from wave-uniform scalars): 32-bit per-lane byte offsets, and the hardware range check returns 0 for the
//   0x80000000 offset given to every position outside the volume -- zero padding costs no compare, no select and no 64-bit
//   address math.
// Everything a thread carries across chunks (xr[], posoff[]; the accumulators its tap block captures) lives in local arrays of
// force-inlined functions and is indexed by unrolled loops only, so it stays in VGPRs: no kernel built on this has a private
// segment.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));     // a 32x32 MFMA accumulator
constexpr int TW = 32;                                          // tile width: one MFMA column block

// Phase cycles of one workgroup (tools/micro/conv_prof.hip builds conv3d.hip with CV_PROFILE); empty otherwise.
// Marks: 0 prologue (tile setup + first chunk's loads issued), 1 commit, 2 MFMA loop (with the next chunk's loads), 3 epilogue.
#ifdef CV_PROFILE
__device__ unsigned long long cv_prof[4 * 4];                   // [wave][mark]
struct StageProf {
    unsigned long long t[4] = {0, 0, 0, 0}, last = clock64();
    __device__ __forceinline__ void mark(int i) { const unsigned long long now = clock64(); t[i] += now - last; last = now; }
};
#else
struct StageProf {
    __device__ __forceinline__ void mark(int) {}
};
#endif

// One workgroup's chunk: an ID x IH x IW halo window (ID = 1: 2-D) of CIC channel planes, NTAPS taps, COP output channels,
// staged by NTHR threads.
template <int ID_, int IH_, int IW_, int CIC_, int NTAPS_, int COP_, int NTHR_ = 256>
struct ConvStage {
    static constexpr int ID = ID_, IH = IH_, IW = IW_, CIC = CIC_, NTAPS = NTAPS_, COP = COP_, NTHR = NTHR_;
    static constexpr int NPOS = ID * IH * IW;                               // halo positions of one channel plane
    static constexpr int PP = (NPOS + NTHR - 1) / NTHR;                     // positions per thread
    static constexpr int NX = CIC * PP;                                     // halo loads per thread and chunk
    static constexpr int XS_FLOATS = CIC * NPOS;                            // [CIC][ID][IH][IW]: the LDS row stride is IW
    static constexpr int WS_FLOATS = NTAPS * CIC * COP;                     // [NTAPS][CIC][COP]
    static constexpr int NWQ = (WS_FLOATS / 4 + NTHR - 1) / NTHR;           // weight float4s per thread
    static constexpr int LDS_BYTES = (XS_FLOATS + 2 * WS_FLOATS) * 4;       // weight slice is double-buffered (LDS-DMA)
    static_assert(CIC % 2 == 0, "k-step is 2 channels");
    static_assert(WS_FLOATS % 4 == 0, "weight slice moves as float4");
};

// Byte offsets of this thread's PP halo positions inside a D x H x W channel plane (HW = H * W); (gz0, gy0, gx0) is the
// window's origin (may be negative).
template <class G>
__device__ __forceinline__ void stage_positions(unsigned (&posoff)[G::PP], int gz0, int gy0, int gx0, int D, int H, int W, int HW,
                                                int tid) {
#pragma unroll
    for (int j = 0; j < G::PP; ++j) {
        const int p = tid + j * G::NTHR;
        int t = p;
        const int xx = t % G::IW; t /= G::IW;
        const int hy = G::ID == 1 ? t : t % G::IH;
        const int dz = G::ID == 1 ? 0 : t / G::IH;
        const int gz = gz0 + dz, gy = gy0 + hy, gx = gx0 + xx;
        const bool ok = p < G::NPOS && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        posoff[j] = ok ? (unsigned)(gz * HW + gy * W + gx) * 4u : 0x80000000u;
    }
}

// The weight slice of the chunk at channel c0 -> wdst.  ws: the packed image [tap][Cw][COP] this workgroup reads; wave_u: the
// wave's index as a scalar (the DMA's LDS address is wave-uniform).
template <class G>
__device__ __forceinline__ void stage_weights(const float* ws, int Cw, int c0, float* wdst, int tid, int wave_u) {
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
    constexpr int TAPQ = G::CIC * G::COP / 4;                               // float4s per tap
#pragma unroll
    for (int i = 0; i < G::NWQ; ++i) {
        const int e = tid + i * G::NTHR;
        if (e < G::WS_FLOATS / 4) {
            const int tap = e / TAPQ, r = e - tap * TAPQ;
            const float* src = ws + ((size_t)tap * Cw + c0) * G::COP + (size_t)r * 4;
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(wdst + (wave_u * 64 + i * G::NTHR) * 4), 16, 0, 0);
        }
    }
}

// Halo load i = cc * PP + j of the chunk at channel c0.  xb: the sample's planes of `plane` floats.  PAD: planes past Ci
// (channel padding of the 3-channel stem) get an empty descriptor: every load returns 0.
template <class G, bool PAD>
__device__ __forceinline__ float stage_load(const float* xb, size_t plane, int Ci, int c0, int i, const unsigned (&posoff)[G::PP]) {
    const int cc = i / G::PP, j = i % G::PP;
    const bool live = !PAD || c0 + cc < Ci;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb + (size_t)(live ? c0 + cc : 0) * plane), 0,
                                                        live ? (unsigned)plane * 4u : 0u, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, posoff[j], 0, 0));
}

// Commit a chunk: xr -> the halo tile Xs, and the chunk's weight DMA has landed.
template <class G>
__device__ __forceinline__ void stage_commit(float* Xs, const float (&xr)[G::NX], int tid) {
    __syncthreads();                                   // previous chunk's LDS reads are done
#pragma unroll
    for (int cc = 0; cc < G::CIC; ++cc)
#pragma unroll
        for (int j = 0; j < G::PP; ++j) {
            const int p = tid + j * G::NTHR;
            if (p < G::NPOS) Xs[cc * G::NPOS + p] = xr[cc * G::PP + j];
        }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's weight DMA for this chunk has landed
    __syncthreads();
}

// The chunk loop.  smem: G::LDS_BYTES of dynamic LDS; tid: threadIdx.x; xb: the sample's Ci planes of D x H x W; the window
// origin as in stage_positions; ws: the packed weights [tap][Cw][COP], Cw (a multiple of CIC) is also where the loop ends.
// tap_mma(tap, Xs, Wc) accumulates one tap of one chunk from the halo tile Xs and the weight slice Wc; it must be
// always_inline so that its accumulators stay in registers, and it is taken by value (see bf16_conv2d.h).
// SPREAD: the next chunk's halo loads are issued LPT per tap inside the MFMA loop -- issued as one burst they fill the memory
// pipeline's queue and the wave sits on it with the matrix core idle (the 3-D kernels); !SPREAD: one burst right after the
// weight DMA (conv2d_mfma).
template <class G, bool SPREAD, bool PAD, class TapMma>
__device__ __forceinline__ void stage_run(float* smem, int tid, const float* xb, int Ci, int gz0, int gy0, int gx0, int D,
                                          int H, int W, const float* ws, int Cw, StageProf& prof, TapMma tap_mma) {
    constexpr int CIC = G::CIC, NX = G::NX, NTAPS = G::NTAPS;
    constexpr int LPT = (NX + NTAPS - 1) / NTAPS;                              // halo loads per tap
    float* Xs = smem;                                  // [CIC][ID][IH][IW]
    float* Ws = smem + G::XS_FLOATS;                   // 2 x [NTAPS][CIC][COP]
    const size_t HW = (size_t)H * W, plane = (size_t)D * HW;
    float xr[NX];
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned posoff[G::PP];
    stage_positions<G>(posoff, gz0, gy0, gx0, D, H, W, (int)HW, tid);
    stage_weights<G>(ws, Cw, 0, Ws, tid, wave_u);
#pragma unroll
    for (int i = 0; i < NX; ++i) xr[i] = stage_load<G, PAD>(xb, plane, Ci, 0, i, posoff);
    prof.mark(0);
    int buf = 0;
    for (int c0 = 0; c0 < Cw; c0 += CIC, buf ^= 1) {
        stage_commit<G>(Xs, xr, tid);
        prof.mark(1);
        const float* Wc = Ws + buf * G::WS_FLOATS;
        const bool more = c0 + CIC < Cw;
        if (more) {
            stage_weights<G>(ws, Cw, c0 + CIC, Ws + (buf ^ 1) * G::WS_FLOATS, tid, wave_u);     // in flight during the MFMA loop below
            if (!SPREAD) {
#pragma unroll
                for (int i = 0; i < NX; ++i) xr[i] = stage_load<G, PAD>(xb, plane, Ci, c0 + CIC, i, posoff);
            }
        }
#pragma unroll
        for (int tap = 0; tap < NTAPS; ++tap) {
            if (SPREAD && more) {
#pragma unroll
                for (int q = 0; q < LPT; ++q)
                    if (tap * LPT + q < NX) xr[tap * LPT + q] = stage_load<G, PAD>(xb, plane, Ci, c0 + CIC, tap * LPT + q, posoff);
            }
            tap_mma(tap, Xs, Wc);
        }
        prof.mark(2);
    }
}

// The launcher tail: 32-bit extent guard (block count; byte offsets inside one channel plane), LDS limit, launch, result.
template <class... P, class... A>
int stage_launch(void (*kern)(P...), long long nblk, unsigned ngrp, int nthr, int lds, long long plane, hipStream_t st, A... args) {
    if (nblk > 0x7fffffffLL || plane * 4 >= 0x80000000LL) return ECM_EUNSUP;
    const hipError_t e = ecm_allow_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk, ngrp), dim3(nthr), lds, st, args...);
    return ECM_LAUNCH_RESULT();
}

}  // namespace
