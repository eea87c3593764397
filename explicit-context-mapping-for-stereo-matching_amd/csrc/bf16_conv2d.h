// The operand staging of the bf16 2-D implicit-GEMM kernels on v_mfma_f32_32x32x16_bf16, written once: conv2d_bf16
// (bf16_encoder.hip) and deconv2d_bf16 (bf16_decoder.hip) are this pipeline around their own MFMA block and epilogue.
//   A k-step is one tap x 16 input channels (a chunk).  The halo tile of a chunk sits in LDS as [position][16 channels] and the
//   chunk's weight slice as [tap][co][16 channels], so one 16-byte LDS read gives a lane (half h = channels 8h .. 8h+7) its
//   whole fragment.  Staging reads whole rows of each channel plane with 16-byte loads (8 positions of one channel; the window
//   is widened to 8-aligned columns), and a thread that holds the same 8 positions of two channels writes them as 8
//   channel-pair words: the [channel][position] -> [position][channel] transpose happens in that write.  Rows of a width that
//   is not a multiple of 8 are not 16-byte aligned: that case (VEC = false) stages the same window with 2-byte loads.
//   Every load is branch-free (an outside position loads the plane's first element and a select zeroes it) and both LDS areas
//   are rounded up to whole 256-thread passes, so no store needs a branch either.
//   The LDS tile is double-buffered: chunk c+1 is written into the other buffer after chunk c's MFMAs, and its global loads
//   (issued one chunk earlier) are in flight under them; one barrier per chunk.
// Everything a thread carries across chunks lives in local arrays of ONE force-inlined function and is indexed by unrolled
// loops only, so it stays in VGPRs: no kernel built on this has a private segment.
#pragma once
#include "common.h"
#include "bf16.h"

namespace {

constexpr int KC = 16;          // input channels per k-step

// Which of the 8 columns gx .. gx+7 of a row are inside a map of width W.  VEC (W % 8 == 0, gx % 8 == 0): a segment is all in
// or all out, one flag; otherwise one bit per column.
template <bool VEC>
__device__ __forceinline__ unsigned mask8(bool row_ok, int gx, int W) {
    unsigned m = 0;
    if (row_ok) {
        if (VEC) m = (unsigned)gx < (unsigned)W ? 0xffu : 0u;
        else
            for (int e = 0; e < 8; ++e) m |= ((unsigned)(gx + e) < (unsigned)W ? 1u : 0u) << e;
    }
    return m;
}

// 8 positions of a row from element offset `off` of a channel plane, masked by mask8's `ok`.  Branch-free, so no load sits
// behind a branch and the compiler can keep all of a thread's loads in flight.  The 2-byte form selects between ADDRESSES
// (plane + off + k or plane), not between indices: the 8 loads then share one base register pair and differ in their
// immediate offset, which is worth 9-68 VGPRs to the kernels that use it.
template <bool VEC>
__device__ __forceinline__ u32x4 load8(const u16* __restrict__ plane, int off, unsigned ok) {
    if (VEC) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(plane + (ok ? off : 0));
        return ok ? v : u32x4{0u, 0u, 0u, 0u};
    }
    unsigned e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool in = (ok >> k) & 1u;
        const unsigned t = *(in ? plane + off + k : plane);
        e[k] = in ? t : 0u;
    }
    return u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}

// One workgroup's tile: HR halo rows of IWP window columns (a multiple of 8), KK taps, COT 32-channel output tiles.
template <int HR, int IWP, int KK, int COT>
struct Stage2d {
    static_assert(IWP % 8 == 0, "the window is whole 8-column segments");
    static constexpr int COLS = IWP, TAPS = KK;
    static constexpr int NSEG = IWP / 8;
    static constexpr int NU = (KC / 2) * HR * NSEG;                               // staging units: channel pair x row x segment
    static constexpr int UPT = (NU + 255) / 256;                                  // units per thread
    static constexpr int HRA = (UPT * 256 + 8 * NSEG - 1) / (8 * NSEG);           // rows allocated: every thread's units land
    static constexpr int XBYTES = HRA * IWP * KC * 2;                             // in LDS, so the staging needs no branch
    static constexpr int COP = COT * 32;
    static constexpr int WQ = KK * COP * 2;                                       // 16-byte vectors of a chunk's weight slice
    static constexpr int WPT = (WQ + 255) / 256;
    static constexpr int BUF = XBYTES + WPT * 256 * 16;                           // the weight area rounded up to whole passes
    static constexpr int LDS_BYTES = 2 * BUF;                                     // what the launch asks for
};

// The chunk loop of a 256-thread workgroup.  xb: the sample's [Ci][H][W] planes; (gy0, gx0): the window's origin in the map
// (gx0 % 8 == 0; may be negative); wp: the weight image [Ci/16][KK][Co][16], of which the workgroup takes output channels
// cb * COP .. + COP.  mma(Xs, Ws) accumulates one chunk from the halo tile Xs and the weight slice Ws (both as uint4 = 8
// channels); it must be always_inline so that its accumulators stay in registers, and it is taken by value: a closure
// passed by reference cost deconv2d_bf16<1, false> an occupancy step.
template <class St, bool VEC, class Mma>
__device__ __forceinline__ void stage2d_run(char* smem, const u16* xb, int Ci, int H, int W, int gy0, int gx0, const u16* wp,
                                            int Co, int cb, Mma mma) {
    constexpr int UPT = St::UPT, WPT = St::WPT, COP = St::COP, WQ = St::WQ;
    const int tid = threadIdx.x;
    const size_t HW = (size_t)H * W;

    // staging unit u: channel pair cp (fastest), segment j, row r
    int uoff[UPT], ulds[UPT];
    unsigned uok[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
        const int u = tid + k * 256;
        const int cp = u & 7, j = (u >> 3) % St::NSEG, r = (u >> 3) / St::NSEG;
        const int gy = gy0 + r, gx = gx0 + 8 * j;
        uok[k] = mask8<VEC>(u < St::NU && (unsigned)gy < (unsigned)H, gx, W);
        uoff[k] = gy * W + gx;                                                     // element offset inside a channel plane
        ulds[k] = ((r * St::COLS + 8 * j) * KC + 2 * cp) * 2;                      // byte offset of position 0, channel 2cp
    }
    u32x4 xr[UPT][2];                                                              // native vectors: promoted to registers,
    u32x4 wr[WPT];                                                                 // unlike uint4 copies
    const int nchunks = Ci / KC;

    auto fetch = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const int cp = (tid + k * 256) & 7;
#pragma unroll
            for (int q = 0; q < 2; ++q) xr[k][q] = load8<VEC>(xb + (size_t)(chunk * KC + 2 * cp + q) * HW, uoff[k], uok[k]);
        }
        // the chunk's weight slice [tap][COP][16] (L2-resident: every workgroup reads the same few KB); with Co == COP and
        // cb == 0 the index folds to a contiguous read
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(wp);
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int e = min(tid + i * 256, WQ - 1);                              // branch-free: the tail re-reads the last vector
            const int hh = e & 1, col = (e >> 1) % COP, t = (e >> 1) / COP;
            wr[i] = wsrc[(((size_t)chunk * St::TAPS + t) * Co + cb * COP + col) * 2 + hh];
        }
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
        char* base = smem + buf * St::BUF;
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {                                          // position e: channels 2cp (low half), 2cp+1
                const unsigned lo = (xr[k][0][e >> 1] >> (16 * (e & 1))) & 0xffffu, hi = (xr[k][1][e >> 1] >> (16 * (e & 1))) & 0xffffu;
                *reinterpret_cast<unsigned*>(base + ulds[k] + e * KC * 2) = lo | (hi << 16);
            }
        }
        u32x4* Ws = reinterpret_cast<u32x4*>(base + St::XBYTES);
#pragma unroll
        for (int i = 0; i < WPT; ++i) Ws[tid + i * 256] = wr[i];                   // past WQ: padding nobody reads
    };

    fetch(0);
    store(0);
    if (nchunks > 1) fetch(1);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        mma(reinterpret_cast<const uint4*>(smem + buf * St::BUF), reinterpret_cast<const uint4*>(smem + buf * St::BUF + St::XBYTES));
        if (ch + 1 < nchunks) {
            store(buf ^ 1);                                                        // the buffer chunk ch-1 used: free since the last barrier
            if (ch + 2 < nchunks) fetch(ch + 2);                                   // in flight under chunk ch+1's MFMAs
        }
        __syncthreads();
    }
}

// Launch the 16-byte-load or the 2-byte-load instantiation (W % 8 == 0 or not) with `lds` bytes of dynamic LDS.
template <class... P, class... A>
int stage2d_launch(void (*kvec)(P...), void (*kany)(P...), bool vec, dim3 grid, int lds, void* stream, A... args) {
    void (*const kern)(P...) = vec ? kvec : kany;
    const hipError_t e = ecm_allow_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, ecm_stream(stream), args...);
    return ECM_LAUNCH_RESULT();
}

// weight image [Ci/16][KK taps][Co][16 channels] bf16 from Conv2d's w [Co,Ci,k,k] or (transposed) ConvTranspose2d's w [Ci,Co,k,k]
__global__ void pack_bf16_2d(const float* __restrict__ w, u16* __restrict__ out, int Ci, int Co, int KK, int transposed) {
    const long long n = (long long)Ci * KK * Co;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i & 15);
    long long r = i >> 4;
    const int co = (int)(r % Co); r /= Co;
    const int t = (int)(r % KK);
    const int ci = (int)(r / KK) * KC + j;
    out[i] = f2bf(w[(transposed ? (size_t)ci * Co + co : (size_t)co * Ci + ci) * KK + t]);
}

int pack_weight_2d(const float* w, u16* packed, int Ci, int Co, int KK, int transposed, void* stream) {
    const long long n = (long long)Ci * KK * Co;
    hipLaunchKernelGGL(pack_bf16_2d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ecm_stream(stream), w, packed, Ci, Co, KK, transposed);
    return ECM_LAUNCH_RESULT();
}

}  // namespace
