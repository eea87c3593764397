// Stereo rectification on the device (include/ecm_rectify.h has the definitions, operation by operation).
//   rectify_map   initUndistortRectifyMap in fp64: one thread per output pixel, the 21 doubles read from a small device buffer
//                 (uniform: scalar loads).  Runs once per rig and device, so nothing here is tuned.
//   remap_pair    the hot path: the raw left and right frames through their maps to the normalised network inputs, both views
//                 and every image in ONE launch (grid z = 2 b + view).  A workgroup is 16 x 16 threads, a thread owns 4
//                 consecutive output columns of one row: a tile of 64 x 16 output pixels, whose source footprint is a compact
//                 patch of the raw frame, so the four taps of neighbouring pixels hit the same cache lines and L1 / L2 do the
//                 gather (no LDS tile).  Outputs are planar: where Wo is a multiple of 4 (and the pointers are 16-byte aligned)
//                 the thread loads its map entries as two float4 and stores one float4 per plane, its four mask bytes as one
//                 word; otherwise every pixel is loaded and stored on its own.
// No atomics, no LDS, no scratch memory; plane offsets are 64-bit.
#include "common.h"
#include "frame_io.h"
#include "../../include/ecm_rectify.h"
#include <climits>
#include <cmath>

namespace {

constexpr int N_PARAMS = 21;                  // iR[9], fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6
constexpr int TX = 16, TY = 16, PX = 4;       // remap_pair: threads of a workgroup in x and y, output columns per thread
constexpr int TILE_W = TX * PX;               // output columns of a workgroup, of both kernels
constexpr int MAP_ROWS = 4;                   // rectify_map: a workgroup is TILE_W x MAP_ROWS threads
constexpr int MAX_SRC_EXTENT = 1 << 24;       // H, W: a tap's column and row are compared as ints converted from fp32
static_assert(TX * TY == 256 && TILE_W * MAP_ROWS == 256, "workgroups of 256 threads");

// ---- the map -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rectify_map(const double* __restrict__ p, float* __restrict__ map, int Ho, int Wo) {
#pragma clang fp contract(off)
    const int ui = blockIdx.x * TILE_W + threadIdx.x, vi = blockIdx.y * MAP_ROWS + threadIdx.y;
    if (ui >= Wo || vi >= Ho) return;
    const double u = (double)ui, v = (double)vi;
    const double X = (p[0] * u + p[1] * v) + p[2];
    const double Y = (p[3] * u + p[4] * v) + p[5];
    const double W = (p[6] * u + p[7] * v) + p[8];
    const double x = X / W, y = Y / W;
    const double fx = p[9], fy = p[10], cx = p[11], cy = p[12];
    const double k1 = p[13], k2 = p[14], p1 = p[15], p2 = p[16], k3 = p[17], k4 = p[18], k5 = p[19], k6 = p[20];
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, r4 = r2 * r2, r6 = r4 * r2, xy2 = 2.0 * (x * y);
    const double radial = (((1.0 + k1 * r2) + k2 * r4) + k3 * r6) / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6);
    const double xd = x * radial + (p1 * xy2 + p2 * (r2 + 2.0 * x2));
    const double yd = y * radial + (p1 * (r2 + 2.0 * y2) + p2 * xy2);
    const size_t plane = (size_t)Ho * Wo, o = (size_t)vi * Wo + ui;
    map[o] = (float)(fx * xd + cx);
    map[plane + o] = (float)(fy * yd + cy);
}

// ---- the remap -----------------------------------------------------------------------------------------------------------------
struct RemapArgs {
    const void *src_l, *src_r;
    const float *map_l, *map_r;
    float *out_l, *out_r, *image;
    unsigned char *mask_l, *mask_r;
    size_t map_stride;                        // floats between the maps of two images: 0 where the batch shares one
    int H, W, Ho, Wo;
    FrameNorm nrm; float border;
};

template <bool U8>
__device__ __forceinline__ float texel(const void* __restrict__ img, size_t hw, size_t pix, int c) {
    if (U8) return (float)static_cast<const unsigned char*>(img)[pix * 3 + c];           // [H,W,3]
    return static_cast<const float*>(img)[(size_t)c * hw + pix];                          // [3,H,W]
}

// s[c] of one output pixel; true where the pixel is inside (mask 1)
template <bool U8>
__device__ __forceinline__ bool sample(const void* __restrict__ img, int H, int W, float mx, float my, float border, float (&s)[3]) {
#pragma clang fp contract(off)
    if (!(fabsf(mx) < __builtin_inff() && fabsf(my) < __builtin_inff())) {
        s[0] = s[1] = s[2] = border;
        return false;
    }
    const float fx0 = floorf(mx), fy0 = floorf(my);
    const float ax = mx - fx0, ay = my - fy0;
    // W, H <= 2^24: beyond the clamp both taps are outside whatever the exact value
    const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)MAX_SRC_EXTENT), y0 = (int)fminf(fmaxf(fy0, -2.f), (float)MAX_SRC_EXTENT);
    const bool l = x0 >= 0 && x0 < W, r = x0 >= -1 && x0 < W - 1, t = y0 >= 0 && y0 < H, b = y0 >= -1 && y0 < H - 1;
    const size_t hw = (size_t)H * W, p00 = (size_t)y0 * W + x0;                           // used only where the tap is inside
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t00 = t && l ? texel<U8>(img, hw, p00, c) : border;
        const float t01 = t && r ? texel<U8>(img, hw, p00 + 1, c) : border;
        const float t10 = b && l ? texel<U8>(img, hw, p00 + W, c) : border;
        const float t11 = b && r ? texel<U8>(img, hw, p00 + W + 1, c) : border;
        const float top = t00 + ax * (t01 - t00), bot = t10 + ax * (t11 - t10);
        s[c] = top + ay * (bot - top);
    }
    return l && r && t && b;
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(TX * TY) void remap_pair(RemapArgs a) {
#pragma clang fp contract(off)
    const int x = (blockIdx.x * TX + threadIdx.x) * PX, y = blockIdx.y * TY + threadIdx.y;
    if (x >= a.Wo || y >= a.Ho) return;
    const int view = blockIdx.z & 1, bi = blockIdx.z >> 1;
    const size_t plane = (size_t)a.Ho * a.Wo, hw = (size_t)a.H * a.W, o = (size_t)y * a.Wo + x;
    const void* src = view ? a.src_r : a.src_l;
    src = U8 ? (const void*)(static_cast<const unsigned char*>(src) + (size_t)bi * hw * 3)
             : (const void*)(static_cast<const float*>(src) + (size_t)bi * hw * 3);
    const float* map = (view ? a.map_r : a.map_l) + (size_t)bi * a.map_stride + o;
    float* out = (view ? a.out_r : a.out_l) + (size_t)bi * 3 * plane + o;
    float* image = view || !a.image ? nullptr : a.image + (size_t)bi * 3 * plane + o;
    unsigned char* mask = view ? a.mask_r : a.mask_l;
    if (mask) mask += (size_t)bi * plane + o;
    const int n = VEC ? PX : (a.Wo - x < PX ? a.Wo - x : PX);

    float mx[PX], my[PX];
    if (VEC) {
        const float4 vx = *reinterpret_cast<const float4*>(map), vy = *reinterpret_cast<const float4*>(map + plane);
        mx[0] = vx.x; mx[1] = vx.y; mx[2] = vx.z; mx[3] = vx.w;
        my[0] = vy.x; my[1] = vy.y; my[2] = vy.z; my[3] = vy.w;
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            mx[k] = k < n ? map[k] : 0.f;
            my[k] = k < n ? map[plane + k] : 0.f;
        }
    }
    float net[3][PX], img[3][PX];                                     // (s / 255 - mean) / std and s / 255
    unsigned inside = 0;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        float s[3] = {0.f, 0.f, 0.f};
        if (k < n) inside |= sample<U8>(src, a.H, a.W, mx[k], my[k], a.border, s) ? 1u << (8 * k) : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            img[c][k] = s[c] / 255.0f;
            net[c][k] = (img[c][k] - a.nrm.mean[c]) / a.nrm.stdv[c];
        }
    }
    if (VEC) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            *reinterpret_cast<float4*>(out + c * plane) = make_float4(net[c][0], net[c][1], net[c][2], net[c][3]);
            if (image) *reinterpret_cast<float4*>(image + c * plane) = make_float4(img[c][0], img[c][1], img[c][2], img[c][3]);
        }
        if (mask) *reinterpret_cast<unsigned*>(mask) = inside;                            // byte k: pixel k (little endian)
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            if (k >= n) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                out[c * plane + k] = net[c][k];
                if (image) image[c * plane + k] = img[c][k];
            }
            if (mask) mask[k] = (inside >> (8 * k)) & 1u;
        }
    }
}

struct Span {
    const char* p;
    size_t n;
};

Span span(const void* p, size_t n) { return Span{static_cast<const char*>(p), n}; }

bool overlap(Span a, Span b) { return a.p && b.p && a.p < b.p + b.n && b.p < a.p + a.n; }

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ecmr_rectify_map_params(void) { return N_PARAMS; }

extern "C" int ecmr_tile_width(void) { return TILE_W; }

extern "C" int ecmr_rectify_map_fwd(const double* params, float* map, int Ho, int Wo, void* stream) {
    ECM_CHECK_ARG(params && map && Ho >= 1 && Wo >= 1 && (const void*)map != (const void*)params);
    if ((long long)Ho * Wo > INT_MAX || Ho > 65535 * MAP_ROWS) return ECM_EUNSUP;
    const size_t map_bytes = (size_t)2 * Ho * Wo * sizeof(float);
    ECM_CHECK_ARG(!overlap(span(map, map_bytes), span(params, N_PARAMS * sizeof(double))));
    const dim3 grid((Wo + TILE_W - 1) / TILE_W, (Ho + MAP_ROWS - 1) / MAP_ROWS), block(TILE_W, MAP_ROWS);
    hipLaunchKernelGGL(rectify_map, grid, block, 0, ecm_stream(stream), params, map, Ho, Wo);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecmr_remap_pair_fwd(const void* left_raw, const void* right_raw, int src_is_u8, const float* map_left,
                                   const float* map_right, int map_per_image, float* left, float* right, float* image,
                                   unsigned char* mask_left, unsigned char* mask_right, int B, int H, int W, int Ho, int Wo,
                                   const float* mean3, const float* std3, float border, void* stream) {
    ECM_CHECK_ARG(left_raw && right_raw && map_left && map_right && left && right && mean3 && std3);
    ECM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && std::isfinite(border));
    for (int c = 0; c < 3; ++c) ECM_CHECK_ARG(std::isfinite(mean3[c]) && std::isfinite(std3[c]) && std3[c] != 0.f);
    const long long hw = (long long)H * W, plane = (long long)Ho * Wo;
    if (B * (hw > plane ? hw : plane) > INT_MAX || H > MAX_SRC_EXTENT || W > MAX_SRC_EXTENT || B > 32767 || Ho > 65535 * TY)
        return ECM_EUNSUP;
    // in place or overlapping: every output against every input and every other output
    const size_t src_bytes = (size_t)B * hw * 3 * (src_is_u8 ? 1 : sizeof(float));
    const size_t map_bytes = (size_t)(map_per_image ? B : 1) * 2 * plane * sizeof(float);
    const size_t out_bytes = (size_t)B * 3 * plane * sizeof(float), mask_bytes = (size_t)B * plane;
    const Span ins[] = {span(left_raw, src_bytes), span(right_raw, src_bytes), span(map_left, map_bytes), span(map_right, map_bytes)};
    const Span outs[] = {span(left, out_bytes), span(right, out_bytes), span(image, out_bytes), span(mask_left, mask_bytes),
                         span(mask_right, mask_bytes)};
    for (int i = 0; i < 5; ++i) {
        for (const Span& in : ins) ECM_CHECK_ARG(!overlap(outs[i], in));
        for (int j = 0; j < i; ++j) ECM_CHECK_ARG(!overlap(outs[i], outs[j]));
    }
    RemapArgs a;
    a.src_l = left_raw; a.src_r = right_raw; a.map_l = map_left; a.map_r = map_right;
    a.out_l = left; a.out_r = right; a.image = image; a.mask_l = mask_left; a.mask_r = mask_right;
    a.map_stride = map_per_image ? (size_t)2 * plane : 0;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.border = border; a.nrm = frame_norm(mean3, std3);
    const bool vec = Wo % PX == 0 && aligned16(map_left) && aligned16(map_right) && aligned16(left) && aligned16(right) &&
                     aligned16(image) && aligned16(mask_left) && aligned16(mask_right);
    const dim3 grid((Wo + TILE_W - 1) / TILE_W, (Ho + TY - 1) / TY, 2 * B), block(TX, TY);
    hipStream_t s = ecm_stream(stream);
#define ECMR_REMAP(u8, v) hipLaunchKernelGGL((remap_pair<u8, v>), grid, block, 0, s, a)
    if (src_is_u8) {
        if (vec) ECMR_REMAP(true, true); else ECMR_REMAP(true, false);
    } else {
        if (vec) ECMR_REMAP(false, true); else ECMR_REMAP(false, false);
    }
#undef ECMR_REMAP
    return ECM_LAUNCH_RESULT();
}
