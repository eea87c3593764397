// Disparity reprojection (include/ecm_geometry.h has the definitions): [X Y Z W]^T = Q_b [x y d 1]^T in
// fp64, the point (X/W, Y/W, Z/W) rounded once to fp32, as a dense map [B,3,H,W] and as a packed cloud of the usable pixels in
// row-major order.  HBM-bound (4-5 B read, 12-28 B written per pixel), so the fp64 arithmetic is free.
// A workgroup owns one linear pixel tile (disp_geom.h): Q is uniform per workgroup, and the pixel order of a tile is (item, wave,
// lane).
//   dense   one launch: every pixel's point or +0.0, and the mask.
//   cloud   three launches, a stable stream compaction:
//     count   the usable pixels of each tile: one ballot per (item, wave), popcounts summed per wave, one int per tile;
//     scan    ONE workgroup walks the B * T counts in chunks of THREADS with a carry: the exclusive scan in place, offsets[b] at
//             each image's first tile, offsets[B] the total;
//     emit    the predicate again, the popcount of each (item, wave) ballot into LDS, one barrier; a pixel's row is its tile's
//             offset + the counts of the (item, wave) pairs before its own + mbcnt of its ballot below its lane.
// No workgroup waits for another (the rule disp_speckle.hip states), no atomics of any kind, no scratch memory: the order is the
// pixel order whatever the scheduling.
#include "disp_geom.h"
#include "../../include/ecm_geometry.h"

namespace {

using namespace ecm_pix;
constexpr int MAX_ATTRS = 4;

typedef unsigned long long u64;

// W of the pixel and whether it is usable; every comparison is on input bits or on the one fp64 value W
__device__ __forceinline__ bool usable(const double* __restrict__ q, float d, bool v, int x, int y, DispRange r, double& w) {
    w = ecm_row4(q + 12, (double)x, (double)y, (double)d);
    return ecm_disp_usable(d, v, r) && ecm_nonzero_finite(w);
}

__device__ __forceinline__ float3 point(const double* __restrict__ q, float d, int x, int y, double w) {
    const double fx = (double)x, fy = (double)y, fd = (double)d;
    const double X = ecm_row4(q, fx, fy, fd), Y = ecm_row4(q + 4, fx, fy, fd), Z = ecm_row4(q + 8, fx, fy, fd);
    return make_float3((float)(X / w), (float)(Y / w), (float)(Z / w));
}

// lanes of the wave below this one that are set in `ballot`
__device__ __forceinline__ int rank_in_wave(u64 ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// ---- dense -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void reproject_dense(const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                           const double* __restrict__ Q, int q_stride, float* __restrict__ xyz,
                                                           unsigned char* __restrict__ mask, int HW, int W, int T, DispRange r) {
    const PixTile t = ecm_pix_tile(T);
    const double* q = Q + (size_t)t.b * q_stride;
    const size_t img = (size_t)t.b * HW;
    float* out = xyz + 3 * img;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned pix = t.first + k * THREADS + threadIdx.x;
        if (pix >= (unsigned)HW) continue;
        const float d = disp[img + pix];
        const bool v = !valid || valid[img + pix] != 0;
        int x, y;
        ecm_pix_xy(pix, W, x, y);
        double w;
        const bool ok = usable(q, d, v, x, y, r, w);
        const float3 p = ok ? point(q, d, x, y, w) : make_float3(0.f, 0.f, 0.f);
        out[pix] = p.x;
        out[(size_t)HW + pix] = p.y;
        out[2 * (size_t)HW + pix] = p.z;
        if (mask) mask[img + pix] = ok ? 1 : 0;
    }
}

// ---- cloud (a): per-tile counts ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void cloud_count(const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                       const double* __restrict__ Q, int q_stride, int* __restrict__ counts,
                                                       int HW, int W, int T, DispRange r) {
    __shared__ int per_wave[NWAVE];
    const PixTile t = ecm_pix_tile(T);
    const double* q = Q + (size_t)t.b * q_stride;
    const size_t img = (size_t)t.b * HW;
    int n = 0;                                                        // wave-uniform: the wave's usable pixels
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned pix = t.first + k * THREADS + threadIdx.x;
        bool ok = false;
        if (pix < (unsigned)HW) {
            const float d = disp[img + pix];
            const bool v = !valid || valid[img + pix] != 0;
            int x, y;
            ecm_pix_xy(pix, W, x, y);
            double w;
            ok = usable(q, d, v, x, y, r, w);
        }
        n += __popcll(__ballot(ok));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) per_wave[threadIdx.x / WAVE] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) sum += per_wave[w];
        counts[blockIdx.x] = sum;
    }
}

// ---- cloud (b): the exclusive scan of the n = B * T counts, in place, by one workgroup -----------------------------------------
__global__ __launch_bounds__(THREADS) void cloud_scan(int* __restrict__ counts, long long* __restrict__ offsets, int n, int T, int B) {
    __shared__ int per_wave[NWAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int carry = 0;                                                    // the sum of every earlier chunk (at most B * H * W < 2^31)
    for (long long base = 0; base < n; base += THREADS) {
        const long long i = base + threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        int s = v;                                                    // inclusive scan within the wave
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int up = __shfl_up(s, off, WAVE);
            if (lane >= off) s += up;
        }
        if (lane == WAVE - 1) per_wave[wave] = s;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            const int c = per_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (i < n) {
            const int excl = carry + before + s - v;
            counts[i] = excl;
            if (i % T == 0) offsets[i / T] = excl;
        }
        carry += total;
        __syncthreads();                                              // per_wave is rewritten by the next chunk
    }
    if (threadIdx.x == 0) offsets[B] = carry;
}

// ---- cloud (c): emit -----------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(THREADS) void cloud_emit(const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                                      const double* __restrict__ Q, int q_stride, const float* __restrict__ attrs,
                                                      const int* __restrict__ tile_offset, float* __restrict__ points,
                                                      float* __restrict__ xyz, unsigned char* __restrict__ mask, int HW, int W, int T,
                                                      DispRange r) {
    __shared__ __align__(16) int count[ITEMS * NWAVE];                // [item][wave]
    static_assert(NWAVE == 4, "an item's counts are read as one int4");
    const PixTile t = ecm_pix_tile(T);
    const double* q = Q + (size_t)t.b * q_stride;
    const size_t img = (size_t)t.b * HW;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;

    float d[ITEMS];
    int below[ITEMS];                                                 // usable lanes of this wave before this one, per item
    unsigned ok_bits = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned pix = t.first + k * THREADS + threadIdx.x;
        bool ok = false;
        d[k] = 0.f;
        if (pix < (unsigned)HW) {
            d[k] = disp[img + pix];
            const bool v = !valid || valid[img + pix] != 0;
            int x, y;
            ecm_pix_xy(pix, W, x, y);
            double w;
            ok = usable(q, d[k], v, x, y, r, w);
        }
        const u64 ballot = __ballot(ok);
        below[k] = rank_in_wave(ballot);
        ok_bits |= ok ? 1u << k : 0u;
        if (lane == 0) count[k * NWAVE + wave] = __popcll(ballot);
    }
    __syncthreads();

    int run = tile_offset[blockIdx.x];                                // rows before item k of this tile
    float* dense = xyz ? xyz + 3 * img : nullptr;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int4 c = reinterpret_cast<const int4*>(count)[k];
        const int before = run + (wave > 0 ? c.x : 0) + (wave > 1 ? c.y : 0) + (wave > 2 ? c.z : 0);
        run += c.x + c.y + c.z + c.w;
        const unsigned pix = t.first + k * THREADS + threadIdx.x;
        if (pix >= (unsigned)HW) continue;
        const bool ok = (ok_bits >> k) & 1u;
        float3 p = make_float3(0.f, 0.f, 0.f);
        if (ok) {
            int x, y;
            ecm_pix_xy(pix, W, x, y);
            const double w = ecm_row4(q + 12, (double)x, (double)y, (double)d[k]);
            p = point(q, d[k], x, y, w);
            float* row = points + (size_t)(before + below[k]) * (3 + C);
            row[0] = p.x;
            row[1] = p.y;
            row[2] = p.z;
#pragma unroll
            for (int a = 0; a < C; ++a) row[3 + a] = attrs[((size_t)t.b * C + a) * HW + pix];
        }
        if (dense) {
            dense[pix] = p.x;
            dense[(size_t)HW + pix] = p.y;
            dense[2 * (size_t)HW + pix] = p.z;
        }
        if (mask) mask[img + pix] = ok ? 1 : 0;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// tiles per image, or 0 where the shape is refused (code: why)
int tiles_per_image(int B, int H, int W, int& code) {
    code = ECM_EINVAL;
    if (B < 1 || H < 1 || W < 1) return 0;
    code = ECM_EUNSUP;
    const long long hw = (long long)H * W;
    if (hw * B > INT_MAX) return 0;           // the batch: the cloud's rows and the scan's carry are ints
    return ecm_pix_tiles(hw, B, code);
}

}  // namespace

extern "C" int ecmg_point_cloud_tile(void) { return TILE; }

extern "C" long long ecmg_point_cloud_scratch_bytes(int B, int H, int W) {
    int code;
    const int T = tiles_per_image(B, H, W, code);
    return T ? (((long long)B * T * (long long)sizeof(int) + 15) / 16) * 16 : 0;
}

extern "C" int ecmg_reproject_fwd(const float* disp, const unsigned char* valid, const double* Q, int q_per_image, float* xyz,
                                  unsigned char* mask, int B, int H, int W, float min_disp, float max_disp, void* stream) {
    ECM_CHECK_ARG(disp && Q && xyz && ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(ecm_no_alias({xyz, mask}, {disp, valid}));
    int code;
    const int T = tiles_per_image(B, H, W, code);
    if (!T) return code;
    const DispRange r = {min_disp, max_disp};
    hipLaunchKernelGGL(reproject_dense, dim3(B * T), dim3(THREADS), 0, ecm_stream(stream), disp, valid, Q, ecm_mat_stride(q_per_image), xyz,
                       mask, H * W, W, T, r);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecmg_point_cloud_fwd(const float* disp, const unsigned char* valid, const double* Q, int q_per_image, const float* attrs,
                                    int C, float* points, long long* offsets, float* xyz, unsigned char* mask, void* scratch,
                                    long long scratch_bytes, int B, int H, int W, float min_disp, float max_disp, void* stream) {
    ECM_CHECK_ARG(disp && Q && points && offsets && scratch && ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(C >= 0 && C <= MAX_ATTRS && (C == 0 || attrs));
    ECM_CHECK_ARG(ecm_no_alias({points, offsets, xyz, mask, scratch}, {disp, valid, Q, attrs}));
    int code;
    const int T = tiles_per_image(B, H, W, code);
    if (!T) return code;
    if (scratch_bytes < ecmg_point_cloud_scratch_bytes(B, H, W)) return ECM_ESCRATCH;
    const DispRange r = {min_disp, max_disp};
    const int HW = H * W, q_stride = ecm_mat_stride(q_per_image), n = B * T;
    int* tiles = static_cast<int*>(scratch);
    hipStream_t s = ecm_stream(stream);
    hipLaunchKernelGGL(cloud_count, dim3(n), dim3(THREADS), 0, s, disp, valid, Q, q_stride, tiles, HW, W, T, r);
    hipLaunchKernelGGL(cloud_scan, dim3(1), dim3(THREADS), 0, s, tiles, offsets, n, T, B);
    return ecm_dispatch<0, 1, 2, 3, 4>(C, [&](auto c) {
        hipLaunchKernelGGL(cloud_emit<decltype(c)::value>, dim3(n), dim3(THREADS), 0, s, disp, valid, Q, q_stride, attrs,
                           (const int*)tiles, points, xyz, mask, HW, W, T, r);
        return ECM_LAUNCH_RESULT();
    });
}
