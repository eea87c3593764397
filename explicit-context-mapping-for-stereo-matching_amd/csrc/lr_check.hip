// Left-right consistency check of two disparity maps (include/ecm_hip.h has the definitions): per pixel
// the error against the right view's disparity warped into the left view, the failure class (0 consistent, 1 occluded,
// 2 mismatch, 3 out of view) and the disparity filled from the nearer-to-background of the nearest consistent columns on the
// left and on the right.  One launch; a workgroup owns a whole row at a time:
//   pass A  columns dealt out thread-interleaved (coalesced): classify, write error and kind, stage d and the scan seed
//           (x where consistent, -1 elsewhere) in LDS;
//   pass B  each thread owns CHUNK consecutive columns of a SWEEP = THREADS * CHUNK: a forward max-scan (nearest consistent
//           column on the left) and a backward min-scan (on the right) -- serial inside the chunk, __shfl_up / __shfl_down inside
//           the wave, the waves' totals through LDS, a running carry from sweep to sweep -- then filled and src into LDS;
//   pass C  filled and src to global memory, thread-interleaved again.
// dr is read straight from global memory: its accesses stay within d columns of the thread's own.
#include "common.h"
#include <climits>

namespace {

constexpr int THREADS = 256, WAVE = 64, NWAVE = THREADS / WAVE;
constexpr int CHUNK = 4;                      // consecutive columns of one thread in the scans (one 16-byte LDS access)
constexpr int SWEEP = THREADS * CHUNK;        // columns the workgroup scans at a time
constexpr int MAX_W = 4096;                   // 4 sweeps; 3 * 4 B of LDS per column: 48 KB + the carries, under the 64 KB default
constexpr int GRID = 512;                     // workgroups of a launch (two per CU); each walks rows GRID apart
constexpr int NONE = INT_MAX;                 // "no consistent column on the right"

__device__ __forceinline__ int pad_width(int W) { return (W + CHUNK - 1) & ~(CHUNK - 1); }

__global__ __launch_bounds__(THREADS) void lr_check_fwd(const float* __restrict__ dl, const float* __restrict__ dr,
                                                        float* __restrict__ check, int* __restrict__ src, long long rows, int W,
                                                        float threshold, float rel, int mirrored) {
    // LDS: tot [2][NWAVE] the waves' scan totals (two sets, used alternately: one barrier per sweep), then per column
    // D the left disparity, L the seed -> nearest consistent column on the left -> src, O filled.  Columns W..Wp-1 pad the last
    // chunk: seed -1, so they are never a source.
    extern __shared__ int lds[];
    const int Wp = pad_width(W);
    int* tot = lds;
    float* D = reinterpret_cast<float*>(lds + 2 * NWAVE);
    int* L = lds + 2 * NWAVE + Wp;
    float* O = reinterpret_cast<float*>(lds + 2 * NWAVE + 2 * Wp);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int nsweep = (W + SWEEP - 1) / SWEEP;
    const size_t plane = (size_t)rows * W;
    const float inf = __builtin_inff(), last = (float)(W - 1);
    int par = 0;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const size_t base = (size_t)row * W;
        const float* dlr = dl + base;
        const float* drr = dr + base;
        float* err = check + base;
        float* kind = err + plane;
        float* fill = kind + plane;

        // ---- pass A: classify
        for (int x = tid; x < Wp; x += THREADS) {
            float d = 0.f;
            int seed = -1;
            if (x < W) {
                d = dlr[x];
                const float xr = (float)x - d;
                float e = inf, k = 3.f;
                if (fabsf(d) < inf && xr >= 0.f && xr <= last) {          // d finite (a NaN fails the comparison) and in view
                    const float f = floorf(xr);
                    const int x0 = (int)f, x1 = min(x0 + 1, W - 1);      // 0 <= x0 <= x1 <= W-1
                    const float r0 = drr[mirrored ? W - 1 - x0 : x0], r1 = drr[mirrored ? W - 1 - x1 : x1];
                    const float r = fmaf(xr - f, r1 - r0, r0);
                    const bool rfin = fabsf(r) < inf;
                    e = rfin ? fabsf(d - r) : inf;
                    k = e <= fmaxf(threshold, rel * d) ? 0.f : (rfin && r > d ? 1.f : 2.f);
                }
                err[x] = e;
                kind[x] = k;
                if (k == 0.f) seed = x;
            }
            D[x] = d;
            L[x] = seed;
        }
        __syncthreads();

        // ---- pass B, forward: L[x] = max{x' <= x : consistent}, -1 for none
        int carry = -1;
        for (int s = 0; s < nsweep; ++s, par ^= 1) {
            const int xc = s * SWEEP + tid * CHUNK;
            int v[CHUNK];
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) v[j] = -1;
            if (xc < Wp) {
                const int4 q = *reinterpret_cast<const int4*>(L + xc);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            }
#pragma unroll
            for (int j = 1; j < CHUNK; ++j) v[j] = max(v[j], v[j - 1]);
            int incl = v[CHUNK - 1];
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const int t = __shfl_up(incl, off, WAVE);
                if (lane >= off) incl = max(incl, t);
            }
            if (lane == WAVE - 1) tot[par * NWAVE + wave] = incl;
            __syncthreads();
            int pre = __shfl_up(incl, 1, WAVE);                           // what precedes this thread's chunk
            if (lane == 0) pre = -1;
            pre = max(pre, carry);
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) {
                const int t = tot[par * NWAVE + w];
                if (w < wave) pre = max(pre, t);
                carry = max(carry, t);
            }
            if (xc < Wp) {
                int4 q;
                q.x = max(v[0], pre); q.y = max(v[1], pre); q.z = max(v[2], pre); q.w = max(v[3], pre);
                *reinterpret_cast<int4*>(L + xc) = q;                     // read again by this thread only
            }
        }

        // ---- pass B, backward: Rx = min{x' >= x : consistent}, NONE for none; then filled and src
        carry = NONE;
        for (int s = nsweep - 1; s >= 0; --s, par ^= 1) {
            const int xc = s * SWEEP + tid * CHUNK;
            int lx[CHUNK], v[CHUNK];
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) lx[j] = -1;
            if (xc < Wp) {
                const int4 q = *reinterpret_cast<const int4*>(L + xc);
                lx[0] = q.x; lx[1] = q.y; lx[2] = q.z; lx[3] = q.w;
            }
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) v[j] = lx[j] == xc + j ? xc + j : NONE;     // consistent: its own nearest on the left
#pragma unroll
            for (int j = CHUNK - 2; j >= 0; --j) v[j] = min(v[j], v[j + 1]);
            int incl = v[0];
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const int t = __shfl_down(incl, off, WAVE);
                if (lane + off < WAVE) incl = min(incl, t);
            }
            if (lane == 0) tot[par * NWAVE + wave] = incl;
            __syncthreads();
            int post = __shfl_down(incl, 1, WAVE);                        // what follows this thread's chunk
            if (lane == WAVE - 1) post = NONE;
            post = min(post, carry);
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) {
                const int t = tot[par * NWAVE + w];
                if (w > wave) post = min(post, t);
                carry = min(carry, t);
            }
            if (xc < Wp) {
                const float4 d4 = *reinterpret_cast<const float4*>(D + xc);
                const float d[CHUNK] = {d4.x, d4.y, d4.z, d4.w};
                float o[CHUNK];
                int from[CHUNK];
#pragma unroll
                for (int j = 0; j < CHUNK; ++j) {
                    const int lxj = lx[j], rxj = min(v[j], post);         // lxj in [-1, W), rxj in [0, W) or NONE
                    if (lxj == xc + j) {
                        o[j] = d[j];
                        from[j] = lxj;
                    } else {
                        const bool hl = lxj >= 0, hr = rxj != NONE;
                        const float a = hl ? D[lxj] : 0.f, b = hr ? D[rxj] : 0.f;
                        const bool right = hr && (!hl || b < a);          // the smaller disparity: the background; the left on a tie
                        o[j] = right ? b : a;
                        from[j] = right ? rxj : lxj;                      // -1 where neither exists (a = 0)
                    }
                }
                *reinterpret_cast<float4*>(O + xc) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<int4*>(L + xc) = make_int4(from[0], from[1], from[2], from[3]);
            }
        }
        __syncthreads();

        // ---- pass C
        for (int x = tid; x < W; x += THREADS) {
            fill[x] = O[x];
            if (src) src[base + x] = L[x];
        }
        __syncthreads();                                                  // the next row overwrites D, L and O
    }
}

}  // namespace

extern "C" int ecm_lr_check_max_width(void) { return MAX_W; }

extern "C" int ecm_lr_check_fwd(const float* dl, const float* dr, float* check, int* src, int B, int H, int W, float threshold,
                                float rel, int mirrored, void* stream) {
    const float inf = __builtin_inff();
    ECM_CHECK_ARG(dl && dr && check && B > 0 && H > 0 && W > 0 && threshold >= 0.f && threshold < inf && rel >= 0.f && rel < inf);
    const long long rows = (long long)B * H;
    if (W > MAX_W || rows > INT_MAX) return ECM_EUNSUP;
    const int Wp = (W + CHUNK - 1) & ~(CHUNK - 1);
    const size_t lds = (2 * NWAVE + 3 * (size_t)Wp) * sizeof(int);
    const int grid = (int)(rows < GRID ? rows : GRID);
    hipLaunchKernelGGL(lr_check_fwd, dim3(grid), dim3(THREADS), lds, ecm_stream(stream), dl, dr, check, src, rows, W, threshold,
                       rel, mirrored);
    return ECM_LAUNCH_RESULT();
}
