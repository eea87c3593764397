// Sparsification curves of K confidence measures against the oracle, per sample, on the device (DESIGN.md section 22;
// include/ecm_hip.h has the definition).  Only `steps` cut ranks of every plane's order are needed, never the order itself, so
// this is a most-significant-digit radix SELECTION over the 32-bit keys, four digits of 8 bits:
//   zero     clears the histograms;
//   hist     one streaming pass per level over pred, gt and the K planes: e, E and bad are formed once per pixel and shared by
//            the K + 1 planes (the last is the oracle, whose key is E).  Level 0 counts the top digit of every valid pixel into a
//            workgroup-private LDS histogram -- float keys crowd into a handful of top digits (sign and exponent), which global
//            atomics would serialise on -- and adds its non-empty bins to the global one.  Levels 1..3 count the next digit of only
//            the pixels whose key starts with one of the at most `steps` prefixes the scan before published ("slots"): the first
//            LDS_SLOTS slots of a sample (through its planes in order) in LDS again -- after one digit of a float nearly every
//            pixel is still under some slot, and there are few -- the rest straight into global memory, where lanes of a wave
//            that meet on one bin (a tie group) are summed in the wave first.
//   scan     one workgroup per (sample, plane): per slot a suffix scan of the 256 bins from the top; every cut finds its bin,
//            adds what lies above it to its running (count, sum E, bad) and keeps the residual rank; the distinct new prefixes
//            become the next level's slots.  The bins read are put back to zero for the next level.  After the last digit the
//            bin of a cut is its tie group, and the same kernel forms the rows.
// A bin is two 64-bit words: count | bad << 32 (both < 2^31: no carry between the halves) and the sum of E (< 2^59).  All
// accumulation is integer addition, which commutes: the same bits every run, and a sample's rows do not depend on its
// neighbours in the batch.  No workgroup waits for another; the order comes from the kernel boundaries.
#include "common.h"
#include <cstdint>

namespace {

typedef unsigned long long u64;

constexpr int ST = 256, PER_THREAD = 8, SPAN = ST * PER_THREAD, MAX_BLOCKS = 256;
constexpr int DIGIT = 8, BINS = 256, LEVELS = 4;
constexpr int MAX_K = 8, MAX_STEPS = 64;
// per (sample, plane) state, in 64-bit words: n, E_tot, bad_tot, slots; per cut prefix | slot << 32, t, n_A, E_A, bad_A; then
// the slot list (32-bit prefixes, descending)
constexpr int ST_HEAD = 4, ST_CUT = 5, ST_WORDS = ST_HEAD + MAX_STEPS * ST_CUT + MAX_STEPS / 2;
constexpr int PEEL_ROUNDS = 2, PEEL_MIN = 4;
// slots of a sample, counted through its planes in order, that a workgroup of the streaming pass counts in LDS: 15 * 4 KB
constexpr int LDS_SLOTS = 15;

struct Planes { const float* m[MAX_K]; };

// The order-preserving image of a measure: -0.0 is +0.0, any NaN is the largest key.
__device__ __forceinline__ unsigned measure_key(float u) {
    unsigned bits = __float_as_uint(u);
    if (u != u) return 0xFFFFFFFFu;
    if (u == 0.f) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__global__ __launch_bounds__(ST) void sparsify_zero(u64* __restrict__ p, long long n) {
    for (long long i = (long long)blockIdx.x * ST + threadIdx.x; i < n; i += (long long)gridDim.x * ST) p[i] = 0;
}

// Add (w0, w1) to bin idx of hist for the lanes that are `on`.  Called by whole waves.  Up to PEEL_ROUNDS times the lanes that
// share the first pending lane's bin are summed in the wave and added once, if there are at least PEEL_MIN of them.
__device__ __forceinline__ void bin_add(u64* __restrict__ hist, bool on, unsigned idx, u64 w0, u64 w1) {
    const int lane = threadIdx.x & 63;
    u64 pending = __ballot(on);
#pragma unroll 1
    for (int round = 0; round < PEEL_ROUNDS && pending; ++round) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned lidx = (unsigned)__shfl((int)idx, leader, 64);
        const bool mine = on && idx == lidx;
        const u64 m = __ballot(mine);
        if (__popcll(m) < PEEL_MIN) break;
        const u64 a0 = wave_sum(mine ? w0 : 0ull), a1 = wave_sum(mine ? w1 : 0ull);
        if (lane == leader) {
            atomicAdd(hist + 2 * (size_t)lidx, a0);
            atomicAdd(hist + 2 * (size_t)lidx + 1, a1);
        }
        on = on && !mine;
        pending &= ~m;
    }
    if (on) {
        atomicAdd(hist + 2 * (size_t)idx, w0);
        atomicAdd(hist + 2 * (size_t)idx + 1, w1);
    }
}

// One pixel, all K + 1 planes.  hist is the sample's global histogram [K+1][steps][BINS][2]; sl / ns are the slot lists (prefixes
// of `done` bits, descending; FIRST: one slot per plane, which every key is under) and sbase[p] the number of slots of the planes
// before p.  Slot sbase[p] + s is counted in the workgroup's LDS histogram lh if it is below LDS_SLOTS, else in global memory.
template <bool FIRST>
__device__ __forceinline__ void sparsify_pixel(float pr, float d, const float (&mv)[MAX_K], bool in, int K, float maxdisp, u64* lh,
                                               u64* __restrict__ hist, const unsigned* sl, const int* ns, const int* sbase, int steps,
                                               int done) {
    const bool valid = in && 0.f < d && d < maxdisp;
    const float e = fabsf(pr - d);
    const float ec = e < 4095.f ? e : 4095.f;                       // a NaN error takes the clamp
    const unsigned E = (unsigned)rintf(ec * 65536.f);               // exact scaling; < 2^28
    const bool bad = !(e < 3.f || e < 0.05f * d);
    const u64 w0 = 1ull | ((u64)(bad ? 1u : 0u) << 32), w1 = E;
#pragma unroll
    for (int p = 0; p <= MAX_K; ++p) {
        if (p > K) continue;
        // the oracle's key is E; shifted up so that its digits spread like a measure's (same order, same groups)
        unsigned key = E << 4;
        if (p < MAX_K && p < K) key = measure_key(mv[p < MAX_K ? p : 0]);
        if (FIRST) {
            if (valid) {                                            // slot p: K + 1 <= LDS_SLOTS
                u64* bin = lh + ((size_t)p * BINS + (key >> (32 - DIGIT))) * 2;
                atomicAdd(bin, w0);
                atomicAdd(bin + 1, w1);
            }
        } else {
            const unsigned prefix = key >> (32 - done);
            const unsigned* list = sl + p * MAX_STEPS;
            int lo = 0, hi = valid ? ns[p] : 0;
            const int n = hi;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (list[mid] > prefix) lo = mid + 1; else hi = mid;
            }
            const bool hit = lo < n && list[lo] == prefix;
            const unsigned digit = (key >> (32 - done - DIGIT)) & (BINS - 1);
            const int g = sbase[p] + lo;
            const bool local = hit && g < LDS_SLOTS;
            if (local) {
                u64* bin = lh + ((size_t)g * BINS + digit) * 2;
                atomicAdd(bin, w0);
                atomicAdd(bin + 1, w1);
            }
            bin_add(hist, hit && !local, ((unsigned)(p * steps + (hit ? lo : 0))) * BINS + digit, w0, w1);
        }
    }
}

// grid (workgroups of a sample, B).  VEC: W % 4 == 0 and every operand 16-byte aligned, so hw % 4 == 0 and a float4 never
// straddles a sample.  Both paths hand every pixel to the same sparsify_pixel.
template <bool VEC, bool FIRST>
__global__ __launch_bounds__(ST) void sparsify_hist(const float* __restrict__ pred, const float* __restrict__ gt, Planes mp, int K,
                                                    u64* __restrict__ hist, const u64* __restrict__ state, int steps, int level,
                                                    unsigned hw, float maxdisp) {
    __shared__ u64 lh[LDS_SLOTS * BINS * 2];
    __shared__ unsigned sl[FIRST ? 1 : (MAX_K + 1) * MAX_STEPS];
    __shared__ int ns[MAX_K + 1], sbase[MAX_K + 2];
    const int tid = threadIdx.x, b = blockIdx.y, P = K + 1;
    const size_t base = (size_t)b * hw;
    u64* hb = hist + (size_t)b * P * steps * BINS * 2;
    for (int q = tid; q < LDS_SLOTS * BINS * 2; q += ST) lh[q] = 0;
    if (FIRST) {
        if (tid <= P) sbase[tid] = tid;
    } else {
        for (int q = tid; q < P * MAX_STEPS; q += ST) {
            const u64* st = state + ((size_t)b * P + q / MAX_STEPS) * ST_WORDS;
            const unsigned* list = reinterpret_cast<const unsigned*>(st + ST_HEAD + MAX_STEPS * ST_CUT);
            const int s = q % MAX_STEPS;
            sl[q] = s < (int)st[3] ? list[s] : 0u;
            if (s == 0) ns[q / MAX_STEPS] = (int)st[3];
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int q = 0; q < P; ++q) { sbase[q] = acc; acc += ns[q]; }
            sbase[P] = acc;
        }
    }
    __syncthreads();
    const int done = level * DIGIT;
    for (unsigned s0 = blockIdx.x * SPAN; s0 < hw; s0 += gridDim.x * SPAN) {
        if (VEC) {
#pragma unroll 1
            for (int k = 0; k < PER_THREAD / 4; ++k) {
                const unsigned i = s0 + (k * ST + tid) * 4;
                const bool in = i < hw;
                float4 pv = {0.f, 0.f, 0.f, 0.f}, dv = pv, m4[MAX_K];
                if (in) { pv = *reinterpret_cast<const float4*>(pred + base + i); dv = *reinterpret_cast<const float4*>(gt + base + i); }
#pragma unroll
                for (int p = 0; p < MAX_K; ++p) {
                    m4[p] = float4{0.f, 0.f, 0.f, 0.f};
                    if (p < K && in) m4[p] = *reinterpret_cast<const float4*>(mp.m[p] + base + i);
                }
                float mv[MAX_K];
#pragma unroll
                for (int p = 0; p < MAX_K; ++p) mv[p] = m4[p].x;
                sparsify_pixel<FIRST>(pv.x, dv.x, mv, in, K, maxdisp, lh, hb, sl, ns, sbase, steps, done);
#pragma unroll
                for (int p = 0; p < MAX_K; ++p) mv[p] = m4[p].y;
                sparsify_pixel<FIRST>(pv.y, dv.y, mv, in, K, maxdisp, lh, hb, sl, ns, sbase, steps, done);
#pragma unroll
                for (int p = 0; p < MAX_K; ++p) mv[p] = m4[p].z;
                sparsify_pixel<FIRST>(pv.z, dv.z, mv, in, K, maxdisp, lh, hb, sl, ns, sbase, steps, done);
#pragma unroll
                for (int p = 0; p < MAX_K; ++p) mv[p] = m4[p].w;
                sparsify_pixel<FIRST>(pv.w, dv.w, mv, in, K, maxdisp, lh, hb, sl, ns, sbase, steps, done);
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < PER_THREAD; ++k) {
                const unsigned i = s0 + k * ST + tid;
                const bool in = i < hw;
                float pr = 0.f, d = 0.f, mv[MAX_K];
                if (in) { pr = pred[base + i]; d = gt[base + i]; }
#pragma unroll
                for (int p = 0; p < MAX_K; ++p) {
                    mv[p] = 0.f;
                    if (p < K && in) mv[p] = mp.m[p][base + i];
                }
                sparsify_pixel<FIRST>(pr, d, mv, in, K, maxdisp, lh, hb, sl, ns, sbase, steps, done);
            }
        }
    }
    __syncthreads();
    const int cached = sbase[P] < LDS_SLOTS ? sbase[P] : LDS_SLOTS;
    for (int q = tid; q < cached * BINS; q += ST) {                 // the non-empty LDS bins go to the sample's histogram
        const u64 w0 = lh[2 * q];
        if (w0) {
            const int g = q / BINS;
            int p = 0;
            while (sbase[p + 1] <= g) ++p;                          // the plane of slot g: g < sbase[P]
            u64* bin = hb + ((size_t)(p * steps + g - sbase[p]) * BINS + q % BINS) * 2;
            atomicAdd(bin, w0);
            atomicAdd(bin + 1, lh[2 * q + 1]);
        }
    }
}

// The row of one cut, in the order of operations the definition gives (fp64, nothing contracted).
__device__ __forceinline__ void sparsify_row(float* __restrict__ out, bool oracle, u64 n, u64 r, u64 Etot, u64 badtot, u64 EA,
                                             u64 badA, u64 t, u64 c, u64 Et, u64 badt) {
#pragma clang fp contract(off)
    if (n == 0) {
        out[0] = out[1] = __builtin_nanf("");
        return;
    }
    const double rest = (double)(long long)(n - r);
    const double remE = (double)(long long)(Etot - EA) - (double)(long long)t * (double)(long long)Et / (double)(long long)c;
    const double rembad = (double)(long long)(badtot - badA) - (double)(long long)t * (double)(long long)badt / (double)(long long)c;
    out[0] = (float)(remE / rest / 65536.0);
    float d1 = (float)(100.0 * rembad / rest);
    if (oracle) d1 = (float)(100.0 * (double)(long long)(badtot - (r < badtot ? r : badtot)) / rest);
    out[1] = d1;
}

// grid (K + 1, B); thread i of the workgroup holds bin BINS-1-i, so that an inclusive scan over the threads counts from the top;
// lane j of wave 0 is cut j.
__global__ __launch_bounds__(ST) void sparsify_scan(u64* __restrict__ hist, u64* __restrict__ state, float* __restrict__ table,
                                                    long long* __restrict__ count, int K, int steps, int level) {
    __shared__ unsigned icnt[BINS], ibad[BINS];
    __shared__ u64 iE[BINS], wt[3][ST / 64];
    const int p = blockIdx.x, b = blockIdx.y, P = K + 1, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    u64* st = state + ((size_t)b * P + p) * ST_WORDS;
    unsigned* list = reinterpret_cast<unsigned*>(st + ST_HEAD + MAX_STEPS * ST_CUT);
    u64* h = hist + ((size_t)b * P + p) * steps * BINS * 2;
    const bool cut = wave == 0 && lane < steps;
    u64 n = 0, Etot = 0, badtot = 0, t = 0, nA = 0, EA = 0, badA = 0, c = 1, Et = 0, badt = 0;
    unsigned prefix = 0;
    int slot = 0, nslots = 1;
    if (level > 0) {
        n = st[0]; Etot = st[1]; badtot = st[2]; nslots = (int)st[3];
        if (cut) {
            const u64* q = st + ST_HEAD + lane * ST_CUT;
            prefix = (unsigned)q[0]; slot = (int)(q[0] >> 32);
            t = q[1]; nA = q[2]; EA = q[3]; badA = q[4];
        }
    }
    for (int s = 0; s < nslots; ++s) {
        u64* bin = h + ((size_t)s * BINS + (BINS - 1 - tid)) * 2;
        const u64 w0 = bin[0], w1 = bin[1];
        bin[0] = 0; bin[1] = 0;                                     // a thread clears the words it read: ready for the next level
        u64 vc = w0 & 0xFFFFFFFFull, vb = w0 >> 32, vE = w1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u64 ac = __shfl_up(vc, off, 64), ab = __shfl_up(vb, off, 64), aE = __shfl_up(vE, off, 64);
            if (lane >= off) { vc += ac; vb += ab; vE += aE; }
        }
        if (lane == 63) { wt[0][wave] = vc; wt[1][wave] = vb; wt[2][wave] = vE; }
        __syncthreads();
        for (int w = 0; w < wave; ++w) { vc += wt[0][w]; vb += wt[1][w]; vE += wt[2][w]; }
        icnt[tid] = (unsigned)vc; ibad[tid] = (unsigned)vb; iE[tid] = vE;
        __syncthreads();
        if (level == 0) {                                           // one slot: the totals of the sample
            n = icnt[BINS - 1]; badtot = ibad[BINS - 1]; Etot = iE[BINS - 1];
            t = (u64)lane * n / (u64)steps;                         // r_j
        }
        if (cut && slot == s && n > 0) {
            int lo = 0, hi = BINS - 1;                              // the first thread whose inclusive count exceeds t
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((u64)icnt[mid] > t) hi = mid; else lo = mid + 1;
            }
            const u64 ac = lo ? icnt[lo - 1] : 0, ab = lo ? ibad[lo - 1] : 0, aE = lo ? iE[lo - 1] : 0;
            c = icnt[lo] - ac; badt = ibad[lo] - ab; Et = iE[lo] - aE;
            nA += ac; badA += ab; EA += aE; t -= ac;
            prefix = (prefix << DIGIT) | (unsigned)(BINS - 1 - lo);
        }
        __syncthreads();
    }
    if (level == 0 && tid == 0) {
        st[0] = n; st[1] = Etot; st[2] = badtot;
        if (p == K) { count[(size_t)b * 3] = (long long)n; count[(size_t)b * 3 + 1] = (long long)Etot; count[(size_t)b * 3 + 2] = (long long)badtot; }
    }
    if (wave != 0) return;
    if (level < LEVELS - 1) {
        const unsigned prev = (unsigned)__shfl_up((int)prefix, 1, 64);
        const bool first = cut && n > 0 && (lane == 0 || prefix != prev);       // the ranks rise with j, so the keys fall
        const u64 m = __ballot(first);
        const int mine = __popcll(m & ((2ull << lane) - 1ull)) - 1;
        if (cut) {
            u64* q = st + ST_HEAD + lane * ST_CUT;
            q[0] = (u64)prefix | ((u64)(unsigned)mine << 32);
            q[1] = t; q[2] = nA; q[3] = EA; q[4] = badA;
        }
        if (first) list[mine] = prefix;
        if (lane == 0) st[3] = (u64)__popcll(m);
    } else if (cut) {
        sparsify_row(table + (((size_t)b * P + p) * steps + lane) * 2, p == K, n, (u64)lane * n / (u64)steps, Etot, badtot, EA, badA,
                     t, c, Et, badt);
    }
}

inline int hist_blocks(long long hw) {
    const long long b = (hw + SPAN - 1) / SPAN;
    return (int)(b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

inline long long hist_words(int B, int K, int steps) { return (long long)B * (K + 1) * steps * BINS * 2; }

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <bool VEC>
void launch_hist(hipStream_t st, int nbx, int B, const float* pred, const float* gt, const Planes& mp, int K, u64* hist,
                 const u64* state, int steps, int level, unsigned hw, float maxdisp) {
    if (level == 0)
        hipLaunchKernelGGL((sparsify_hist<VEC, true>), dim3(nbx, B), dim3(ST), 0, st, pred, gt, mp, K, hist, state, steps, level, hw, maxdisp);
    else
        hipLaunchKernelGGL((sparsify_hist<VEC, false>), dim3(nbx, B), dim3(ST), 0, st, pred, gt, mp, K, hist, state, steps, level, hw, maxdisp);
}

}  // namespace

extern "C" int ecm_eval_sparsify_max_measures(void) { return MAX_K; }
extern "C" int ecm_eval_sparsify_max_steps(void) { return MAX_STEPS; }

extern "C" long long ecm_eval_sparsify_scratch_bytes(int B, int H, int W, int K, int steps) {
    if (B < 1 || H < 1 || W < 1 || K < 1 || K > MAX_K || steps < 1 || steps > MAX_STEPS) return 0;
    if (B > 65535 || (long long)H * W > 0x7fffffffLL) return 0;
    return (hist_words(B, K, steps) + (long long)B * (K + 1) * ST_WORDS) * (long long)sizeof(u64);
}

extern "C" int ecm_eval_sparsify(const float* pred, const float* gt, const float* const* measures, float* table, long long* count,
                                 void* scratch, long long scratch_bytes, int B, int H, int W, int K, int steps, float maxdisp,
                                 void* stream) {
    ECM_CHECK_ARG(pred && gt && measures && table && count && scratch && B >= 1 && H >= 1 && W >= 1 && K >= 1 && steps >= 1);
    ECM_CHECK_ARG(reinterpret_cast<uintptr_t>(scratch) % 8 == 0);
    const long long hw = (long long)H * W;
    if (hw > 0x7fffffffLL || B > 65535 || K > MAX_K || steps > MAX_STEPS) return ECM_EUNSUP;
    Planes mp = {};
    bool vec = W % 4 == 0 && aligned16(pred) && aligned16(gt);
    for (int k = 0; k < K; ++k) {
        ECM_CHECK_ARG(measures[k]);
        mp.m[k] = measures[k];
        vec = vec && aligned16(measures[k]);
    }
    if (scratch_bytes < ecm_eval_sparsify_scratch_bytes(B, H, W, K, steps)) return ECM_ESCRATCH;
    u64* hist = static_cast<u64*>(scratch);
    const long long nh = hist_words(B, K, steps);
    u64* state = hist + nh;
    hipStream_t st = ecm_stream(stream);
    const int nbx = hist_blocks(hw);
    const long long zb = (nh + ST * 8 - 1) / (ST * 8);
    hipLaunchKernelGGL(sparsify_zero, dim3((unsigned)(zb > 1024 ? 1024 : zb)), dim3(ST), 0, st, hist, nh);
    for (int level = 0; level < LEVELS; ++level) {
        if (vec) launch_hist<true>(st, nbx, B, pred, gt, mp, K, hist, state, steps, level, (unsigned)hw, maxdisp);
        else launch_hist<false>(st, nbx, B, pred, gt, mp, K, hist, state, steps, level, (unsigned)hw, maxdisp);
        hipLaunchKernelGGL(sparsify_scan, dim3(K + 1, B), dim3(ST), 0, st, hist, state, table, count, K, steps, level);
    }
    return ECM_LAUNCH_RESULT();
}
