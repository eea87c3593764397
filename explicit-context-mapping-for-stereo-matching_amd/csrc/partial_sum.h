// The fixed-order sum of per-workgroup partials, stated once: the second stage of every weight gradient whose persistent
// workgroups each leave one partial (conv3d_wgrad.hip, conv3d_c1.hip, ecm_weights_bwd.hip).  Deterministic, no float atomics.
// A workgroup of 256 owns 32 outputs; its 8 lane groups each sum every 8th partial and the 8 group sums are added in order.
// (One thread per output walking all the partials was latency-bound: up to 1024 partials x a few thousand outputs.)
// Additions only, in one order: whoever calls these gets the same bits.
//
// Deliberately NOT folded in here, because their order of additions differs and moving them would change bits:
//   c1_reduce (conv2d_c1.hip)       4 waves x 64 outputs, two accumulators, and it splits the bias off the last output
//   chsum_final (conv2d_c1.hip)     one workgroup per channel over a wave shuffle tree
//   the loss, eval and GroupNorm finals (loss.hip, eval.hip, gn3d.hip): fp64 or Welford merges of their own
#pragma once
#include "common.h"

namespace {

// lane group grp's share of sum_p src[p * stride], p = grp, grp + 8, ... < n
__device__ __forceinline__ float partial_group_sum(const float* __restrict__ src, size_t stride, int n, int grp) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = grp;
    for (; p + 24 < n; p += 32) {
        s0 += src[(size_t)p * stride];
        s1 += src[(size_t)(p + 8) * stride];
        s2 += src[(size_t)(p + 16) * stride];
        s3 += src[(size_t)(p + 24) * stride];
    }
    for (; p < n; p += 8) s0 += src[(size_t)p * stride];
    return (s0 + s1) + (s2 + s3);
}

// the workgroup tail: every thread hands in its group's sum s of output column o (0 for a dead column); group 0 adds the eight
// in order and stores the live ones.  Called by all 256 threads.
__device__ __forceinline__ void partial_tail(float s, int o, int grp, bool live, float* __restrict__ dst) {
    __shared__ float sm[8][32];
    sm[grp][o] = s;
    __syncthreads();
    if (grp == 0 && live) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += sm[g][o];
        *dst = t;
    }
}

// out[i] = sum_p partial[p][i], i < n, over P partials of n floats each; grid = (n + 31) / 32 workgroups of 256
// (a template only so that a file that includes this header for the two helpers carries no copy of the kernel)
template <int = 0>
__global__ __launch_bounds__(256) void ecm_sum_partials(const float* __restrict__ partial, float* __restrict__ out, int n, int P) {
    const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    partial_tail(i < n ? partial_group_sum(partial + i, (size_t)n, P, grp) : 0.f, o, grp, i < n, out + i);
}

}  // namespace
