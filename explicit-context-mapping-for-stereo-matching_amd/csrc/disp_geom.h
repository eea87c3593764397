// Disparity-space geometry and tile plumbing, stated once for the kernels that work on a disparity map:
// disp_reproject.hip, disp_warp.hip, motion_align.hip, disp_volume.hip, disp_filter.hip, disp_speckle.hip and disp_wls.hip.
// No entry points.  What is here is what the public headers call THE rule: a kernel that restates one of these is a second copy
// that nothing holds to the first.
#pragma once
#include "common.h"
#include <climits>
#include <cmath>
#include <initializer_list>

// ---- values ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ecm_finite(double v) { return fabs(v) < __builtin_inf(); }
__device__ __forceinline__ bool ecm_finite(float v) { return fabsf(v) < __builtin_inff(); }
// what a homogeneous coordinate has to be before anything is divided by it
__device__ __forceinline__ bool ecm_nonzero_finite(double w) { return fabs(w) < __builtin_inf() && w != 0.0; }

// One row of a 4x4 matrix on (a, b, c, 1), as include/ecm_geometry.h defines it: ((m0 a + m1 b) + m2 c) + m3, every product and
// sum one fp64 operation in that order.  The pragma is in the body, so no fused multiply-add is formed whatever the including
// file does: the bit-exactness that ecm_geometry.h, ecm_temporal.h, ecm_motion.h and ecm_volume.h state rests on this function.
__device__ __forceinline__ double ecm_row4(const double* __restrict__ m, double a, double b, double c) {
#pragma clang fp contract(off)
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3];
}

struct DispRange {
    float lo, hi;                             // usable: lo < d <= hi
};

// the usable-disparity rule of include/ecm_geometry.h: comparisons on input bits only
__device__ __forceinline__ bool ecm_disp_usable(float d, bool v, DispRange r) {
    return v && fabsf(d) < __builtin_inff() && d > r.lo && d <= r.hi;
}

// d at `at`, or NaN where it is not finite or not valid: then every comparison with it is false
__device__ __forceinline__ float ecm_disp_or_nan(const float* __restrict__ d, const unsigned char* __restrict__ valid, size_t at) {
    float v = d[at];
    if (!(fabsf(v) < __builtin_inff()) || (valid && valid[at] == 0)) v = __builtin_nanf("");
    return v;
}

// ---- the linear pixel tile -------------------------------------------------------------------------------------------------------
// TILE = THREADS x ITEMS consecutive pixels (or lattice pixels) of ONE image; a workgroup owns one tile, so whatever is indexed
// by the image is uniform per workgroup.  Item k of thread t is pixel k * THREADS + t of the tile: a wave reads 64 consecutive
// pixels at a time.
namespace ecm_pix {
constexpr int THREADS = 256, WAVE = 64, NWAVE = THREADS / WAVE;
constexpr int ITEMS = 8;                      // pixels of a tile per thread: eight independent loads in flight
constexpr int TILE = THREADS * ITEMS;
constexpr int MAX_TILES = 16777215;           // B * T: the launch's global size (tiles x THREADS) stays below 2^32
}  // namespace ecm_pix

struct PixTile {
    int b;                                    // image
    unsigned first;                           // first pixel of the tile within the image
};

// the tile of this workgroup, of T tiles per image
__device__ __forceinline__ PixTile ecm_pix_tile(int T) {
    PixTile t;
    t.b = (int)(blockIdx.x / (unsigned)T);
    t.first = (blockIdx.x % (unsigned)T) * (unsigned)ecm_pix::TILE;
    return t;
}

__device__ __forceinline__ void ecm_pix_xy(unsigned pix, int W, int& x, int& y) {
    y = (int)(pix / (unsigned)W);
    x = (int)(pix - (unsigned)y * (unsigned)W);
}

// Tiles per image for `items` pixels in each of B images; 0, with code = ECM_EUNSUP, where the launch would pass MAX_TILES.  The
// caller's own size rules come first.
static inline int ecm_pix_tiles(long long items, int B, int& code) {
    const long long T = (items + ecm_pix::TILE - 1) / ecm_pix::TILE;
    code = T * B > ecm_pix::MAX_TILES ? ECM_EUNSUP : 0;
    return code ? 0 : (int)T;
}

// ---- the 2-D tile walk: tiles of TW x TH pixels, image after image -----------------------------------------------------------------
struct Tiles2D {
    int tx, ty;                               // tiles along x and y
    long long n;                              // B * tx * ty
};

template <int TW, int TH>
__host__ __device__ inline Tiles2D ecm_tiles_of(int B, int H, int W) {
    Tiles2D t;
    t.tx = (W + TW - 1) / TW;
    t.ty = (H + TH - 1) / TH;
    t.n = (long long)B * t.tx * t.ty;
    return t;
}

// ---- host-side operand rules -------------------------------------------------------------------------------------------------------
static inline bool ecm_disp_range_ok(float min_disp, float max_disp) {
    return std::isfinite(min_disp) && !std::isnan(max_disp) && max_disp >= min_disp;
}

static inline bool ecm_positive(float v) { return std::isfinite(v) && v > 0.f; }

// doubles between the 4x4 matrices of consecutive images: one matrix each, or one shared by all
static inline int ecm_mat_stride(int per_image) { return per_image ? 16 : 0; }

// no output that was passed is one of the inputs (a null pointer is an operand that was not passed)
static inline bool ecm_no_alias(std::initializer_list<const void*> outs, std::initializer_list<const void*> ins) {
    for (const void* o : outs)
        for (const void* i : ins)
            if (o && o == i) return false;
    return true;
}
