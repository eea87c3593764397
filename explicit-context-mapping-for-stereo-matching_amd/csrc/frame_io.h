// What the decodes of resident frames share (frame_prep.hip, frame_jitter.hip, rectify.hip): the operands of
// a launch chunk, the loads of a packed shard and the host's window checks.  NO floating-point arithmetic: frame_jitter.hip needs
// contraction off, and arithmetic inlined from a header was fused (section 37).  uint8 -> float and half -> float are exact.
#pragma once
#include <hip/hip_fp16.h>
#include <type_traits>

constexpr int FP_MAXB = 32;                   // samples whose window origins one launch carries
struct FrameCrops { int y0[FP_MAXB], x0[FP_MAXB]; };
struct FrameNorm { float mean[3], stdv[3]; };
inline FrameNorm frame_norm(const float* m, const float* s) { return FrameNorm{{m[0], m[1], m[2]}, {s[0], s[1], s[2]}}; }
// all B windows of rows x cols lie inside the H x W frame (the loader's randint bounds); 64-bit: no origin wraps into the frame
inline bool frame_windows_inside(const int* y0, const int* x0, int B, int rows, int cols, int H, int W) {
    for (int b = 0; b < B; ++b)
        if (!(y0[b] >= 0 && x0[b] >= 0 && (long long)y0[b] + rows <= H && (long long)x0[b] + cols <= W)) return false;
    return true;
}
// the origins of samples [b0, b0 + nb), nb <= FP_MAXB, as a launch takes them
inline FrameCrops frame_crops(const int* y0, const int* x0, int b0, int nb) {
    FrameCrops c{};
    for (int i = 0; i < nb; ++i) { c.y0[i] = y0[b0 + i]; c.x0[i] = x0[b0 + i]; }
    return c;
}
// one view's RGB of pixel `pix` of a packed shard's uint8 [B,H,W,6] (left RGB, right RGB): 6 B per pixel, so three 16-bit loads
template <class T>
__device__ __forceinline__ void frame_unpack3(const unsigned char* rgb6, size_t pix, bool right, T* c) {
    const unsigned short* p = reinterpret_cast<const unsigned short*>(rgb6 + pix * 6);
    const int a = p[0], b = p[1], e = p[2];
    if (right) { c[0] = (T)(b >> 8); c[1] = (T)(e & 0xff); c[2] = (T)(e >> 8); }
    else { c[0] = (T)(a & 0xff); c[1] = (T)(a >> 8); c[2] = (T)(b & 0xff); }
}
template <bool HALF>                          // a packed shard's disparity, fp16 | fp32 [B,H,W]
__device__ __forceinline__ float frame_disp(const void* disp, size_t pix) {
    return HALF ? __half2float(static_cast<const __half*>(disp)[pix]) : static_cast<const float*>(disp)[pix];
}
template <class F>                            // f(std::true_type) for an fp16 disparity, f(std::false_type) for fp32
int frame_by_disp(int disp_is_half, F&& f) { return disp_is_half ? f(std::true_type{}) : f(std::false_type{}); }
