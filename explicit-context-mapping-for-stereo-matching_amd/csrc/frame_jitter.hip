// The training transform of the reference's KITTI loader (cmf/loader/KITTI.py:144-191) inside the decode of a packed frame, and
// its colour jitter alone on resident uint8 images (include/ecm_augment.h states every operation).
//   KITTI.transform, train branch, per view: ToPILImage -> ColorJitter(0.4, 0.4, 0.4, 0.4) -> ToTensor -> Lighting (a PCA shift
//   of three floats) -> clamp(0, 1) -> Normalize.  The float round trip into the PIL image is the identity on 0..255, so the PIL
//   image holds the frame's own bytes, and ColorJitter is up to four Pillow operations on uint8 RGB, each on the result of the
//   one before it, in a shuffled order: ImageEnhance.Brightness / Contrast / Color (a blend with black, with the rounded mean of
//   the gray image, with the pixel's own gray) and an HSV round trip with a shifted hue.
// Contrast needs the mean gray of the view as it stands when contrast is reached, so a view with contrast takes two launches: a
// reduction that runs the operations in front of contrast and leaves one INTEGER partial sum per tile in caller scratch, and the
// apply launch, whose workgroups each add their view's partials (integers: the same sum in any order), run all operations per
// pixel and write the outputs in one pass.  No atomics, no zeroing pass, no float sums.
// The arithmetic is Pillow's, operation for operation, and a fused multiply-add changes bytes (DESIGN.md section 37 counts how
// many), so contraction is off for this file and every fp32 step goes through add_rn .. div_rn below.  They are defined HERE,
// behind the pragma: HIP's __fmul_rn / __fadd_rn are a plain `x * y` / `x + y` in a header compiled with contraction allowed, and
// a product and a sum inlined from there are fused all the same (that changed 84 bytes of a 37x53 contrast at factor 0.6).
#include "common.h"
#include "../../include/ecm_augment.h"
#include "frame_io.h"

#pragma clang fp contract(off)

namespace {

constexpr int JT_MAXV = 2 * FP_MAXB;          // views per launch chunk: both views of frame_io.h's FP_MAXB samples
constexpr int JT_THREADS = 256, JT_PPT = 8, JT_TILE = JT_THREADS * JT_PPT;
constexpr long long JT_MAX_PIXELS = 1ll << 24;        // S <= 255 * 2^24 < 2^32, and PIL's int(mean + 0.5) is exact up to here
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3, OP_NONE = 15;

// ops: four nibbles (the codes in order, OP_NONE behind them), the hue shift in bits 16..23, bit 24 set where contrast is present
struct JitterViews { float f[JT_MAXV][3]; float pca[JT_MAXV][3]; int ops[JT_MAXV]; };
constexpr int HAS_CONTRAST = 1 << 24;

struct RGB { int r, g, b; };

__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }      // IEEE: hipcc's fp32 division is correctly rounded

__device__ __forceinline__ int gray_of(RGB p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }

__device__ __forceinline__ int blend1(float d, int a, float f) {
    const float t = add_rn(d, mul_rn(f, sub_rn((float)a, d)));
    return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}
__device__ __forceinline__ RGB blend(float d, RGB p, float f) { return RGB{blend1(d, p.r, f), blend1(d, p.g, f), blend1(d, p.b, f)}; }

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
__device__ __forceinline__ int round8(float x) { return clip8((int)floorf(add_rn(x, 0.5f))); }

__device__ __forceinline__ RGB hue_op(RGB p, int shift) {
    const int mx = max(max(p.r, p.g), p.b), mn = min(min(p.r, p.g), p.b);
    int uh = 0, us = 0;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = div_rn(cr, (float)mx);
        const float rc = div_rn((float)(mx - p.r), cr), gc = div_rn((float)(mx - p.g), cr), bc = div_rn((float)(mx - p.b), cr);
        float h;
        if (p.r == mx) h = sub_rn(bc, gc);
        else if (p.g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        double hd = (double)h / 6.0 + 1.0;              // in [5/6, 11/6]: fmod(hd, 1.0) is hd - floor(hd), exactly
        hd = hd - floor(hd);
        h = (float)hd;
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) return RGB{mx, mx, mx};
    const float v = (float)mx;
    const float fs = div_rn((float)us, 255.f);
    float f = div_rn(mul_rn((float)uh, 6.f), 255.f);
    const float fi = floorf(f);
    f = sub_rn(f, fi);
    const int pp = round8(mul_rn(v, sub_rn(1.f, fs)));
    const int q = round8(mul_rn(v, sub_rn(1.f, mul_rn(fs, f))));
    const int t = round8(mul_rn(v, sub_rn(1.f, mul_rn(fs, sub_rn(1.f, f)))));
    const int i = (int)fi;                              // 0..6; 6 (h = 255) is sector 0 again
    if (i == 1) return RGB{q, mx, pp};
    if (i == 2) return RGB{pp, mx, t};
    if (i == 3) return RGB{pp, q, mx};
    if (i == 4) return RGB{t, pp, mx};
    if (i == 5) return RGB{mx, pp, q};
    return RGB{mx, t, pp};
}

// The view's operations on one pixel, in order.  UNTIL_CONTRAST: only those in front of contrast (the reduction's prefix).
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ RGB run_ops(RGB p, int ops, float fb, float fc, float fsat, int m) {
    const int shift = (ops >> 16) & 255;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int code = (ops >> (4 * k)) & 15;         // uniform over the workgroup: these are scalar branches
        if (code == OP_NONE) break;
        if (code == OP_BRIGHTNESS) p = blend(0.f, p, fb);
        else if (code == OP_CONTRAST) {
            if (UNTIL_CONTRAST) break;
            p = blend((float)m, p, fc);
        } else if (code == OP_SATURATION) p = blend((float)gray_of(p), p, fsat);
        else if (code == OP_HUE) p = hue_op(p, shift);
    }
    return p;
}

// Sum of one unsigned per thread over the workgroup, returned to every thread.
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = JT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// ---- where a view's pixels come from.  gv: the view's index in the whole call, lv: in the launch chunk.
struct SrcFrame {                     // packed frames: uint8 [B,H,W,6] (view 2b = left, 2b+1 = right of sample b), a window each
    const unsigned char* rgb;
    FrameCrops crops;
    int H, W, tw;
    __device__ __forceinline__ size_t pixel(int gv, int lv, int p) const {
        const int bl = lv >> 1, r = p / tw, x = p - r * tw;
        return ((size_t)(gv >> 1) * H + (crops.y0[bl] + r)) * W + (crops.x0[bl] + x);
    }
    __device__ __forceinline__ RGB load(size_t pix, int gv) const {
        int c[3];
        frame_unpack3(rgb, pix, gv & 1, c);
        return RGB{c[0], c[1], c[2]};
    }
};
struct SrcU8 {                        // resident views: uint8 [N,H,W,3]
    const unsigned char* img;
    size_t n;
    __device__ __forceinline__ size_t pixel(int gv, int, int p) const { return (size_t)gv * n + p; }
    __device__ __forceinline__ RGB load(size_t pix, int) const {
        const unsigned char* q = img + pix * 3;
        return RGB{q[0], q[1], q[2]};
    }
};

// ---- where they go
template <bool HALF>
struct SinkFrame {                    // KITTI.py:171-191 behind the jitter: NCHW fp32, coalesced per plane
    float *left, *right, *disp, *image;
    const void* disp_in;
    FrameNorm nrm;
    size_t plane;
    __device__ __forceinline__ void store(int gv, int p, size_t pix, RGB c, float s0, float s1, float s2) const {
        const int b = gv >> 1, side = gv & 1;
        const size_t o = (size_t)b * 3 * plane + p;
        float* dst = side ? right : left;
        const int u[3] = {c.r, c.g, c.b};
        const float sh[3] = {s0, s1, s2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float x = add_rn(div_rn((float)u[k], 255.f), sh[k]);
            x = fminf(fmaxf(x, 0.f), 1.f);
            if (!side && image) image[o + k * plane] = x;                                       // KITTI.py:189: the clamped left view
            dst[o + k * plane] = div_rn(sub_rn(x, nrm.mean[k]), nrm.stdv[k]);
        }
        if (!side) disp[(size_t)b * plane + p] = frame_disp<HALF>(disp_in, pix);
    }
};
struct SinkU8 {
    unsigned char* out;
    __device__ __forceinline__ void store(int, int, size_t pix, RGB c, float, float, float) const {
        unsigned char* q = out + pix * 3;
        q[0] = (unsigned char)c.r; q[1] = (unsigned char)c.g; q[2] = (unsigned char)c.b;
    }
};

// grid (tiles, views of a sample, samples of the chunk): one workgroup per tile of JT_TILE pixels of one view
__device__ __forceinline__ int local_view() { return blockIdx.z * gridDim.y + blockIdx.y; }

template <class Src>
__global__ __launch_bounds__(JT_THREADS) void jitter_reduce_kernel(Src src, JitterViews jv, unsigned* __restrict__ partial, int n,
                                                                   int tiles, int v0) {
    __shared__ unsigned red[JT_THREADS];
    const int lv = local_view(), gv = v0 + lv, ops = jv.ops[lv];
    if (!(ops & HAS_CONTRAST)) return;                  // uniform: the whole workgroup leaves
    const float fb = jv.f[lv][0], fsat = jv.f[lv][2];
    unsigned sum = 0;
#pragma unroll 1
    for (int k = 0; k < JT_PPT; ++k) {
        const int p = blockIdx.x * JT_TILE + k * JT_THREADS + threadIdx.x;
        if (p < n) sum += gray_of(run_ops<true>(src.load(src.pixel(gv, lv, p), gv), ops, fb, 0.f, fsat, 0));
    }
    sum = block_sum(sum, red);
    if (threadIdx.x == 0) partial[(size_t)gv * tiles + blockIdx.x] = sum;
}

template <class Src, class Sink>
__global__ __launch_bounds__(JT_THREADS) void jitter_apply_kernel(Src src, Sink sink, JitterViews jv, const unsigned* __restrict__ partial,
                                                                  int n, int tiles, int v0) {
    __shared__ unsigned red[JT_THREADS];
    const int lv = local_view(), gv = v0 + lv, ops = jv.ops[lv];
    int m = 0;
    if (ops & HAS_CONTRAST) {                           // uniform
        // a partial is at most 2048 * 255 and the view's sum at most 255 * 2^24 < 2^32: unsigned holds both
        unsigned s = 0;
        for (int i = threadIdx.x; i < tiles; i += JT_THREADS) s += partial[(size_t)gv * tiles + i];
        const unsigned long long S = block_sum(s, red);
        m = (int)((2 * S + (unsigned long long)n) / (2 * (unsigned long long)n));
    }
    const float fb = jv.f[lv][0], fc = jv.f[lv][1], fsat = jv.f[lv][2];
    const float s0 = jv.pca[lv][0], s1 = jv.pca[lv][1], s2 = jv.pca[lv][2];
#pragma unroll 1
    for (int k = 0; k < JT_PPT; ++k) {
        const int p = blockIdx.x * JT_TILE + k * JT_THREADS + threadIdx.x;
        if (p < n) {
            const size_t pix = src.pixel(gv, lv, p);
            sink.store(gv, p, pix, run_ops<false>(src.load(pix, gv), ops, fb, fc, fsat, m), s0, s1, s2);
        }
    }
}

// ---- host side
int jitter_tiles(long long n) { return (int)((n + JT_TILE - 1) / JT_TILE); }

long long scratch_bytes_of(int views, int rows, int cols) {
    if (views < 1 || rows < 1 || cols < 1 || rows > 65535 || (long long)rows * cols > JT_MAX_PIXELS) return 0;
    return (long long)views * jitter_tiles((long long)rows * cols) * 4;
}

// The parameters of the views [v0, v0 + nv) as the kernels take them; false for an order that is not distinct codes 0..3 followed
// by -1s, or a shift outside 0..255.
bool pack_views(JitterViews& jv, int v0, int nv, const float* factors, const int* order, const int* hue_shift, const float* pca,
                bool& any_contrast) {
    for (int i = 0; i < nv; ++i) {
        const int v = v0 + i;
        int ops = 0, seen = 0;
        bool ended = false;
        for (int k = 0; k < 4; ++k) {
            const int code = order[4 * v + k];
            if (code == -1) { ended = true; ops |= OP_NONE << (4 * k); continue; }
            if (ended || code < 0 || code > 3 || (seen >> code & 1)) return false;
            seen |= 1 << code;
            ops |= code << (4 * k);
        }
        if (hue_shift[v] < 0 || hue_shift[v] > 255) return false;
        ops |= hue_shift[v] << 16;
        if (seen >> OP_CONTRAST & 1) { ops |= HAS_CONTRAST; any_contrast = true; }
        jv.ops[i] = ops;
        for (int c = 0; c < 3; ++c) { jv.f[i][c] = factors[3 * v + c]; jv.pca[i][c] = pca ? pca[3 * v + c] : 0.f; }
    }
    return true;
}

// per_sample views of a sample (1: resident views, 2: the two views of a frame); total views, n pixels each
template <class MakeSrc, class Sink>
int jitter_launch(MakeSrc make_src, Sink sink, int views, int per_sample, long long n, const float* factors, const int* order,
                  const int* hue_shift, const float* pca, unsigned* partial, hipStream_t st) {
    const int tiles = jitter_tiles(n);
    {   // every view's parameters are checked before the first launch
        JitterViews jv{};
        bool any = false;
        for (int v0 = 0; v0 < views; v0 += JT_MAXV)
            if (!pack_views(jv, v0, views - v0 < JT_MAXV ? views - v0 : JT_MAXV, factors, order, hue_shift, pca, any)) return ECM_EINVAL;
    }
    for (int v0 = 0; v0 < views; v0 += JT_MAXV) {
        const int nv = views - v0 < JT_MAXV ? views - v0 : JT_MAXV;
        JitterViews jv{};
        bool any_contrast = false;
        pack_views(jv, v0, nv, factors, order, hue_shift, pca, any_contrast);
        auto src = make_src(v0, nv);
        const dim3 grid(tiles, per_sample, nv / per_sample), block(JT_THREADS);
        if (any_contrast)
            hipLaunchKernelGGL((jitter_reduce_kernel<decltype(src)>), grid, block, 0, st, src, jv, partial, (int)n, tiles, v0);
        hipLaunchKernelGGL((jitter_apply_kernel<decltype(src), Sink>), grid, block, 0, st, src, sink, jv, partial, (int)n, tiles, v0);
    }
    return ECM_LAUNCH_RESULT();
}

}  // namespace

extern "C" int ecma_jitter_tile(void) { return JT_TILE; }

extern "C" long long ecma_jitter_scratch_bytes(int views, int rows, int cols) { return scratch_bytes_of(views, rows, cols); }

extern "C" int ecma_color_jitter_fwd(const unsigned char* images, unsigned char* out, int N, int H, int W, const float* factors,
                                     const int* order, const int* hue_shift, void* scratch, long long scratch_bytes, void* stream) {
    ECM_CHECK_ARG(images && out && factors && order && hue_shift && scratch && N > 0 && H > 0 && W > 0 && images != out);
    const long long n = (long long)H * W;
    if (H > 65535 || n > JT_MAX_PIXELS) return ECM_EUNSUP;
    if (scratch_bytes < scratch_bytes_of(N, H, W)) return ECM_ESCRATCH;
    auto make_src = [=](int, int) { return SrcU8{images, (size_t)n}; };
    return jitter_launch(make_src, SinkU8{out}, N, 1, n, factors, order, hue_shift, nullptr, static_cast<unsigned*>(scratch),
                         ecm_stream(stream));
}

extern "C" int ecma_frame_prep_jitter_fwd(const unsigned char* rgb6, const void* disp_in, int disp_is_half, float* left, float* right,
                                          float* disp, float* image, int B, int H, int W, const int* crop_y0, const int* crop_x0, int th,
                                          int tw, const float* factors, const int* order, const int* hue_shift, const float* pca,
                                          const float* mean3, const float* std3, void* scratch, long long scratch_bytes, void* stream) {
    ECM_CHECK_ARG(rgb6 && disp_in && left && right && disp && crop_y0 && crop_x0 && factors && order && hue_shift && pca && mean3 &&
                  std3 && scratch && B > 0 && H > 0 && W > 0 && th > 0 && tw > 0);
    if (th > 65535 || (long long)th * tw > JT_MAX_PIXELS || B > (1 << 29)) return ECM_EUNSUP;
    if (!frame_windows_inside(crop_y0, crop_x0, B, th, tw, H, W)) return ECM_EINVAL;
    if (scratch_bytes < scratch_bytes_of(2 * B, th, tw)) return ECM_ESCRATCH;
    auto make_src = [=](int v0, int nv) { return SrcFrame{rgb6, frame_crops(crop_y0, crop_x0, v0 / 2, nv / 2), H, W, tw}; };
    return frame_by_disp(disp_is_half, [&](auto half) {
        const SinkFrame<decltype(half)::value> sink{left, right, disp, image, disp_in, frame_norm(mean3, std3), (size_t)th * tw};
        return jitter_launch(make_src, sink, 2 * B, 2, (long long)th * tw, factors, order, hue_shift, pca, static_cast<unsigned*>(scratch),
                             ecm_stream(stream));
    });
}
