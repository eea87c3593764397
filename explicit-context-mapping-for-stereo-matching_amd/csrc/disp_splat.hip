// Forward warp ("splat") of a left disparity map into the right view (include/ecm_hip.h has the
// definitions): every finite, in-view pixel x of a row lands on the one or two right-view columns about x - d -- the columns
// lr_check.hip's pass A reads for it -- and per right column the candidate with the largest disparity wins, the larger source
// column among equals: the nearest surface hides what lies behind it.  One launch; a workgroup owns a whole row at a time:
//   pass A  columns dealt out thread-interleaved (coalesced): build the packed key and take an LDS atomic max of it on x0 and,
//           where x - d is not integral, on x1;
//   pass B  thread-interleaved again: decode the winner, write right and src, and put the LDS word back to 0 for the next row
//           (a thread clears exactly the words it read, so one barrier per pass is enough).
// The key: the high 32 bits are the order-preserving image of the float's bits (all bits flipped where the sign bit is set, else
// the sign bit set: unsigned order is float order, with -0.0 below +0.0), the low 32 bits the source column.  Every finite
// float's image is >= 0x00800000, so the word 0 is "nothing landed here".
// The only atomics are integer maxima in LDS: the result does not depend on the order of arrival and is bit-reproducible.  No
// global atomics, no scratch memory.
#include "common.h"
#include <climits>

namespace {

constexpr int THREADS = 256;
constexpr int MAX_W = 4096;                   // one 8-byte LDS word per column: 32 KB, under the 64 KB default
constexpr int GRID = 512;                     // workgroups of a launch (two per CU); each walks rows GRID apart

typedef unsigned long long u64;

__global__ __launch_bounds__(THREADS) void disp_splat_fwd(const float* __restrict__ dl, float* __restrict__ right,
                                                          int* __restrict__ src, long long rows, int W) {
    extern __shared__ u64 best[];             // [W]: the winning key of each right-view column, 0 for none
    const int tid = threadIdx.x;
    const float inf = __builtin_inff(), last = (float)(W - 1);

    for (int x = tid; x < W; x += THREADS) best[x] = 0;
    __syncthreads();

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const size_t base = (size_t)row * W;
        const float* dlr = dl + base;

        // ---- pass A: splat
        for (int x = tid; x < W; x += THREADS) {
            const float d = dlr[x];
            const float xr = (float)x - d;
            if (fabsf(d) < inf && xr >= 0.f && xr <= last) {             // d finite (a NaN fails the comparison) and in view
                const float f = floorf(xr);
                const int x0 = (int)f;                                    // 0 <= x0 <= W-1
                const unsigned bits = __float_as_uint(d);
                const unsigned image = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
                const u64 key = ((u64)image << 32) | (unsigned)x;
                atomicMax(&best[x0], key);
                if (xr > f) atomicMax(&best[min(x0 + 1, W - 1)], key);   // xr > f implies x0 < W-1
            }
        }
        __syncthreads();

        // ---- pass B: decode, store, clear
        for (int x = tid; x < W; x += THREADS) {
            const u64 key = best[x];
            best[x] = 0;
            const unsigned image = (unsigned)(key >> 32);
            const unsigned bits = (image & 0x80000000u) ? (image ^ 0x80000000u) : ~image;
            right[base + x] = key ? __uint_as_float(bits) : 0.f;
            if (src) src[base + x] = key ? (int)(unsigned)key : -1;
        }
        __syncthreads();                                                  // the next row splats into the cleared words
    }
}

}  // namespace

extern "C" int ecm_disp_splat_max_width(void) { return MAX_W; }

extern "C" int ecm_disp_splat_fwd(const float* dl, float* right, int* src, int B, int H, int W, void* stream) {
    ECM_CHECK_ARG(dl && right && right != dl && (const void*)src != (const void*)dl && B > 0 && H > 0 && W > 0);
    const long long rows = (long long)B * H;
    if (W > MAX_W || rows > INT_MAX) return ECM_EUNSUP;
    const size_t lds = (size_t)W * sizeof(u64);
    const int grid = (int)(rows < GRID ? rows : GRID);
    hipLaunchKernelGGL(disp_splat_fwd, dim3(grid), dim3(THREADS), lds, ecm_stream(stream), dl, right, src, rows, W);
    return ECM_LAUNCH_RESULT();
}
