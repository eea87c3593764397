// Neighbour sets of the context-mapping weight generators, shared by the forward and backward kernels and by the disparity
// heads that consume the weights: Nbr<0> is the eight-neighbour head's table (heads.hip, head_stats.hip, head_mode.hip), Nbr<1>
// the volume-mapping head's five-neighbour fuse (variants.hip).
// VAR 0: eight_related (cmfsm.py:431-593): 9 planes c,l,r,t,b,lt,rt,lb,rb; tables 0,1,2,3,4,1,2,3,4
//   (5..8 alias 1..4, cmfsm.py:459-462, quirk Q2); out-of-image logit -100; output softmax.
// VAR 1: six_related, reference image (cmfsm_sub_8.py:449-572): 5 planes c,r,l,t,b with tables 0,1,2,3,4
//   (right uses table 1, left table 2: cmfsm_sub_8.py:503,525); out-of-image logit 0 (still in the softmax);
//   extra LeakyReLU after conv3 (:318,342); output softmax*logit (:572).
// VAR 2: six_related, target image: 3 planes c,r,l (cmfsm_sub_8.py:483-536), same MLP on the right-image features.
#pragma once
#include <hip/hip_runtime.h>

template <int VAR> struct Nbr;
template <> struct Nbr<0> {
    static constexpr int N = 9; static constexpr bool FINAL_ACT = false, TIMES_LOGIT = false;
    static constexpr float PAD = -100.f;
    static __device__ __forceinline__ int dy(int n) { constexpr int t[9] = {0, 0, 0, -1, 1, -1, -1, 1, 1}; return t[n]; }
    static __device__ __forceinline__ int dx(int n) { constexpr int t[9] = {0, -1, 1, 0, 0, -1, 1, -1, 1}; return t[n]; }
    static __device__ __forceinline__ int tab(int n) { constexpr int t[9] = {0, 1, 2, 3, 4, 1, 2, 3, 4}; return t[n]; }
};
template <> struct Nbr<1> {
    static constexpr int N = 5; static constexpr bool FINAL_ACT = true, TIMES_LOGIT = true;
    static constexpr float PAD = 0.f;
    static __device__ __forceinline__ int dy(int n) { constexpr int t[5] = {0, 0, 0, -1, 1}; return t[n]; }
    static __device__ __forceinline__ int dx(int n) { constexpr int t[5] = {0, 1, -1, 0, 0}; return t[n]; }
    static __device__ __forceinline__ int tab(int n) { constexpr int t[5] = {0, 1, 2, 3, 4}; return t[n]; }
};
template <> struct Nbr<2> {
    static constexpr int N = 3; static constexpr bool FINAL_ACT = true, TIMES_LOGIT = true;
    static constexpr float PAD = 0.f;
    static __device__ __forceinline__ int dy(int n) { return 0; }
    static __device__ __forceinline__ int dx(int n) { constexpr int t[3] = {0, 1, -1}; return t[n]; }
    static __device__ __forceinline__ int tab(int n) { constexpr int t[3] = {0, 1, 2}; return t[n]; }
};

// The mixture an HR pixel of the eight-neighbour head draws from the LR cells around (cy, cx) (head_stats.hip, head_mode.hip):
// cell[n] = the LR cell of neighbour n, -1 where aggregate9_fwd skips it (outside the image), and a[n] = w9[n] / sum of the
// valid w9, 0 for a skipped neighbour.  w9p points at plane 0 of the pixel's nine weights, HW apart.
__device__ __forceinline__ void ecm_mixture9(const float* __restrict__ w9p, long long HW, int cy, int cx, int h, int w,
                                             float (&a)[9], int (&cell)[9]) {
    float wsum = 0.f;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const int yy = cy + Nbr<0>::dy(n), xx = cx + Nbr<0>::dx(n);
        const bool ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
        cell[n] = ok ? yy * w + xx : -1;
        a[n] = ok ? w9p[(size_t)n * HW] : 0.f;
        wsum += a[n];
    }
    const float inv = 1.f / wsum;
#pragma unroll
    for (int n = 0; n < 9; ++n) a[n] *= inv;
}

__device__ __forceinline__ float ecm_centre_pat(int r, int s) { return (float)(r < s / 2 ? r - s / 2 : r - s / 2 + 1); }
// offset channel 0 (varies with X) / channel 1 (varies with Y) of table t at in-cell position r
__device__ __forceinline__ float ecm_off_x(int t, int r, int s) {
    return t == 1 ? (float)(s - r) : t == 2 ? (float)(r + 1) : ecm_centre_pat(r, s);
}
__device__ __forceinline__ float ecm_off_y(int t, int r, int s) {
    return t == 3 ? (float)(s - r) : t == 4 ? (float)(r + 1) : ecm_centre_pat(r, s);
}
