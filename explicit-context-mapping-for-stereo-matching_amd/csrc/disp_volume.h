// The per-voxel update and the per-ray march of the TSDF volume, stated once (include/ecm_volume.h has the definitions) for
// disp_volume.hip and disp_color.hip.  No entry points.  The colour kernels run the same projection, the same tsdf update and the
// same march, and add their own arithmetic through a functor: what they leave in tsdf, wsum, out and hit_weight is what
// disp_volume.hip leaves there because it is this code, not a copy of it.
// Everything here is compiled with contraction off, and so is whatever follows in the including file: every product and sum is
// one IEEE operation, as the headers state them.
#pragma once
#include "disp_geom.h"
#include <cstdint>
#include <initializer_list>

#pragma clang fp contract(off)

namespace ecm_vol {

constexpr int THREADS = 256;
constexpr int BRICK_X = 16, BRICK_Y = 4, BRICK_Z = 4;     // threads of a brick; BRICK_X * VEC voxels along x
constexpr int TILE = 16;                                  // pixels of a raycast tile, each way
constexpr int MAX_GROUPS = 16777215;                      // workgroups of a launch: its global size stays below 2^32
constexpr int MAX_STEPS = 65536;

struct Gates {
    DispRange range;
    float max_weight;
    double trunc;
};

// ---- integrate -----------------------------------------------------------------------------------------------------------------
// one view's update of one voxel: X = tsdf, N = wsum.  Where the view is not skipped, seen(pix, w, s) is called with the pixel the
// voxel projects to (0 <= pix < H * W), its weight and s = z_meas - z_vox; it touches neither X nor N.
template <class Seen>
__device__ __forceinline__ void integrate_view(float& X, float& N, double di, double dj, double dk, const double* __restrict__ G,
                                               const double* __restrict__ Cm, const double* __restrict__ Q,
                                               const float* __restrict__ disp, const unsigned char* __restrict__ valid,
                                               const float* __restrict__ weight, int H, int W, const Gates& g, Seen&& seen) {
    const double h3 = ecm_row4(G + 12, di, dj, dk);
    const double u = ecm_row4(G, di, dj, dk) / h3, v = ecm_row4(G + 4, di, dj, dk) / h3, dv = ecm_row4(G + 8, di, dj, dk) / h3;
    if (!(ecm_finite(u) && ecm_finite(v) && ecm_finite(dv) && dv > 0.0)) return;
    const double fx = floor(u + 0.5), fy = floor(v + 0.5);
    if (!(fx >= 0.0 && fx <= (double)(W - 1) && fy >= 0.0 && fy <= (double)(H - 1))) return;
    const size_t pix = (size_t)(int)fy * W + (int)fx;                       // 0 <= pix < H * W
    const float d = disp[pix];
    if (!ecm_disp_usable(d, !valid || valid[pix] != 0, g.range)) return;
    const float w = weight ? weight[pix] : 1.f;
    if (!(w > 0.f && w < __builtin_inff())) return;
    const double fd = (double)d;
    const double P3 = ecm_row4(Q + 12, fx, fy, fd);
    if (!ecm_nonzero_finite(P3)) return;
    const double z_meas = ecm_row4(Q + 8, fx, fy, fd) / P3;
    const double z_vox = ecm_row4(Cm + 8, di, dj, dk);
    if (!(ecm_finite(z_meas) && z_meas > 0.0 && ecm_finite(z_vox) && z_vox > 0.0)) return;
    const double s = z_meas - z_vox;
    if (s < -g.trunc) return;
    const float t = (float)fmin(1.0, s / g.trunc);
    const float Wn = N + w;
    X = (X * N + t * w) / Wn;
    N = fminf(Wn, g.max_weight);
    seen(pix, w, s);
}

// the voxels of one thread of a brick: i0 is its first voxel along x, `at` the linear index of (i0, j, k); false: it has none
struct Voxels {
    long long i0;
    int j, k;
    size_t at;
};

template <int VEC>
__device__ __forceinline__ bool brick_voxels(Voxels& o, int nx, int ny, int nz, int bx, int by) {
    const unsigned blk = blockIdx.x;
    const int bi = (int)(blk % (unsigned)bx), bj = (int)((blk / (unsigned)bx) % (unsigned)by), bk = (int)(blk / ((unsigned)bx * (unsigned)by));
    const int tx = threadIdx.x & (BRICK_X - 1), ty = (threadIdx.x / BRICK_X) & (BRICK_Y - 1), tz = threadIdx.x / (BRICK_X * BRICK_Y);
    o.i0 = ((long long)bi * BRICK_X + tx) * VEC;                            // bx * BRICK_X * VEC may pass nx by a brick: below 2^32
    o.j = bj * BRICK_Y + ty, o.k = bk * BRICK_Z + tz;
    if (o.i0 >= nx || o.j >= ny || o.k >= nz) return false;                 // VEC == 4: nx % 4 == 0, so i0 + 3 < nx as well
    o.at = ((size_t)o.k * ny + o.j) * nx + (size_t)o.i0;                    // below nx * ny * nz < 2^31
    return true;
}

// VEC consecutive values of a plane: one 16-byte access where VEC == 4 (the caller saw to the alignment)
template <int VEC>
__device__ __forceinline__ void load_voxels(float (&r)[VEC], const float* __restrict__ p) {
    if constexpr (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w;
    } else {
        r[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void store_voxels(float* __restrict__ p, const float (&r)[VEC]) {
    if constexpr (VEC == 4)
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else
        p[0] = r[0];
}

// the bricks of a launch for nx * ny * nz voxels, VEC of them per thread; false where the launch would pass MAX_GROUPS
struct Bricks {
    long long bx, by, bz;
};

static inline bool bricks_of(Bricks& b, int nx, int ny, int nz, int vec) {
    const long long per = (long long)BRICK_X * vec;
    b.bx = (nx + per - 1) / per, b.by = (ny + BRICK_Y - 1) / BRICK_Y, b.bz = (nz + BRICK_Z - 1) / BRICK_Z;
    return b.bx * b.by * b.bz <= MAX_GROUPS;
}

// ---- raycast -------------------------------------------------------------------------------------------------------------------
struct Cell {
    int x, y, z;                              // the lower corner
    double qx, qy, qz;                        // the position within the cell
};

// the cell min(max(floor(p), 0), dim-2) about a point, and the point's position within it
__device__ __forceinline__ Cell cell_about(double px, double py, double pz, int nx, int ny, int nz) {
    const double wx = fmin(fmax(floor(px), 0.0), (double)(nx - 2)), wy = fmin(fmax(floor(py), 0.0), (double)(ny - 2));
    const double wz = fmin(fmax(floor(pz), 0.0), (double)(nz - 2));
    return {(int)wx, (int)wy, (int)wz, px - wx, py - wy, pz - wz};
}

// the header's blend of the eight values of `plane` about the cell, widened
__device__ __forceinline__ double blend(const float* __restrict__ plane, const Cell& c, int nx, int ny) {
    const float* __restrict__ p = plane + ((size_t)c.z * ny + c.y) * nx + c.x;
    const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
    const double t000 = p[0], t001 = p[1], t010 = p[sy], t011 = p[sy + 1];
    const double t100 = p[sz], t101 = p[sz + 1], t110 = p[sz + sy], t111 = p[sz + sy + 1];
    const double a00 = t000 + c.qx * (t001 - t000), a01 = t010 + c.qx * (t011 - t010);
    const double a10 = t100 + c.qx * (t101 - t100), a11 = t110 + c.qx * (t111 - t110);
    const double e0 = a00 + c.qy * (a01 - a00), e1 = a10 + c.qy * (a11 - a10);
    return e0 + c.qz * (e1 - e0);
}

__device__ __forceinline__ bool all_weighted(const float* __restrict__ wsum, const Cell& c, int nx, int ny) {
    const float* __restrict__ p = wsum + ((size_t)c.z * ny + c.y) * nx + c.x;
    const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
    return p[0] > 0.f && p[1] > 0.f && p[sy] > 0.f && p[sy + 1] > 0.f && p[sz] > 0.f && p[sz + 1] > 0.f && p[sz + sy] > 0.f
        && p[sz + sy + 1] > 0.f;
}

// narrow [s_lo, s_hi] to where gn + dir * s can lie in [0, top) on one axis; false: it lies there for no s.  A direction too
// small for the margin of one sample to cover the rounding of a sample's own position gives no constraint at all.
__device__ __forceinline__ bool clip_axis(double gn, double dir, double top, double& s_lo, double& s_hi) {
    if (dir == 0.0) return gn >= 0.0 && gn < top;                           // every sample is gn itself
    if (!(fabs(dir) * 1073741824.0 > fabs(gn) + top)) return true;
    const double s0 = (0.0 - gn) / dir, s1 = (top - gn) / dir;
    s_lo = fmax(s_lo, fmin(s0, s1));
    s_hi = fmin(s_hi, fmax(s0, s1));
    return true;
}

// the pixel of this thread in a launch of tiles of TILE x TILE pixels, each wave on 8 x 8 of them; false: outside the image
struct Ray {
    int b;
    long long x, y;
    size_t pix;                               // (b, y, x) in a [B,H,W] plane
};

__device__ __forceinline__ bool tile_ray(Ray& r, int H, int W, int tiles_x, int tiles) {
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    r.b = (int)(blockIdx.x / (unsigned)tiles);
    r.x = (long long)(tile % tiles_x) * TILE + (wave & 1) * 8 + (lane & 7);
    r.y = (long long)(tile / tiles_x) * TILE + (wave >> 1) * 8 + (lane >> 3);
    if (r.x >= W || r.y >= H) return false;
    r.pix = (size_t)r.b * H * W + (size_t)r.y * W + (size_t)r.x;
    return true;
}

// the tiles of a raycast of B views; false where the launch would pass MAX_GROUPS
struct RayTiles {
    long long x, per_view;
};

static inline bool ray_tiles_of(RayTiles& t, int B, int H, int W) {
    t.x = ((long long)W + TILE - 1) / TILE;
    t.per_view = t.x * (((long long)H + TILE - 1) / TILE);
    return t.per_view * B <= MAX_GROUPS;
}

struct March {
    double near_disp, far_disp, step;
    int max_steps;
};

// The march of pixel (fx, fy) through the volume with the matrices R and Ri of its view: result is the disparity of the hit and,
// where want_weight, weight the blend of wsum there; both stay +0.0 for a hole.  At a hit, hit(qx, qy, qz) is called with p*.
template <class Hit>
__device__ __forceinline__ void march_ray(float& result, float& weight, const float* __restrict__ tsdf, const float* __restrict__ wsum,
                                          const double* __restrict__ R, const double* __restrict__ Ri, double fx, double fy, int nx, int ny,
                                          int nz, const March& mr, bool want_weight, Hit&& hit) {
    const double near_disp = mr.near_disp, far_disp = mr.far_disp;
    const double hn = ecm_row4(R + 12, fx, fy, near_disp), hf = ecm_row4(R + 12, fx, fy, far_disp);
    const double gx = ecm_row4(R, fx, fy, near_disp) / hn, gy = ecm_row4(R + 4, fx, fy, near_disp) / hn, gz = ecm_row4(R + 8, fx, fy, near_disp) / hn;
    const double ex = ecm_row4(R, fx, fy, far_disp) / hf, ey = ecm_row4(R + 4, fx, fy, far_disp) / hf, ez = ecm_row4(R + 8, fx, fy, far_disp) / hf;
    const double dx = ex - gx, dy = ey - gy, dz = ez - gz;
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    const double nd = ceil(len / mr.step);
    const bool ends = ecm_finite(gx) && ecm_finite(gy) && ecm_finite(gz) && ecm_finite(ex) && ecm_finite(ey) && ecm_finite(ez);
    if (!(ends && nd >= 1.0 && nd <= (double)mr.max_steps)) return;         // a NaN fails both comparisons
    const int n = (int)nd;
    double s_lo = 0.0, s_hi = 1.0;
    bool some = clip_axis(gx, dx, (double)(nx - 1), s_lo, s_hi) && clip_axis(gy, dy, (double)(ny - 1), s_lo, s_hi)
        && clip_axis(gz, dz, (double)(nz - 1), s_lo, s_hi);
    some = some && s_lo <= s_hi + 2.0 / nd;                                 // so both are finite: -2/n <= s_hi, s_lo <= 1 + 2/n
    int m_lo = 0, m_hi = -1;
    if (some) {
        m_lo = max((int)floor(s_lo * nd) - 1, 0);
        m_hi = min((int)ceil(s_hi * nd) + 1, n);
    }
    bool before = false;                                                    // the sample before this one was valid
    double f0 = 0.0, px0 = 0.0, py0 = 0.0, pz0 = 0.0;
#pragma unroll 1
    for (int m = m_lo; m <= m_hi; ++m) {
        const double s = (double)m / nd;
        const double px = gx + dx * s, py = gy + dy * s, pz = gz + dz * s;
        const double cx = floor(px), cy = floor(py), cz = floor(pz);
        bool ok = cx >= 0.0 && cx <= (double)(nx - 2) && cy >= 0.0 && cy <= (double)(ny - 2) && cz >= 0.0 && cz <= (double)(nz - 2);
        double f = 0.0;
        if (ok) {
            const Cell c = {(int)cx, (int)cy, (int)cz, px - cx, py - cy, pz - cz};
            ok = all_weighted(wsum, c, nx, ny);
            if (ok) f = blend(tsdf, c, nx, ny);
        }
        if (ok && before) {
            if (f0 > 0.0 && f <= 0.0) {
                const double a = f0 / (f0 - f);
                const double qx = px0 + (px - px0) * a, qy = py0 + (py - py0) * a, qz = pz0 + (pz - pz0) * a;
                result = (float)(ecm_row4(Ri + 8, qx, qy, qz) / ecm_row4(Ri + 12, qx, qy, qz));
                if (want_weight) weight = (float)blend(wsum, cell_about(qx, qy, qz, nx, ny, nz), nx, ny);
                hit(qx, qy, qz);
                break;
            }
            if (f0 < 0.0 && f > 0.0) break;                                 // a back face
        }
        before = ok;
        f0 = f, px0 = px, py0 = py, pz0 = pz;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static inline bool voxels_fit(int nx, int ny, int nz) { return (long long)nx * ny * nz <= INT_MAX; }   // after nx, ny, nz >= 1: nx * ny <= 2^62

// the sizes a volume and an image must have for the kernels' index arithmetic
static inline bool sizes_fit(int nx, int ny, int nz, int H, int W) {
    return (long long)nx * ny <= INT_MAX && voxels_fit(nx, ny, nz) && (long long)H * W <= INT_MAX;
}

// The launch of an integration, after the entry's own argument checks: VEC = 4 where nx % 4 == 0 and every plane the kernel updates
// in place (`planes`) is 16-byte aligned, else 1; the bricks of that VEC, their number and the gates.  false: unsupported sizes.
struct IntegratePlan {
    int vec;
    Bricks bricks;
    Gates gates;
    unsigned groups;
};

static inline bool integrate_plan(IntegratePlan& p, int nx, int ny, int nz, int H, int W, float trunc, float max_weight, float min_disp,
                                  float max_disp, std::initializer_list<const void*> planes) {
    if (!sizes_fit(nx, ny, nz, H, W)) return false;
    uintptr_t low = 0;
    for (const void* plane : planes) low |= (uintptr_t)plane;
    p.vec = nx % 4 == 0 && low % 16 == 0 ? 4 : 1;
    if (!bricks_of(p.bricks, nx, ny, nz, p.vec)) return false;
    p.gates = {{min_disp, max_disp}, max_weight, (double)trunc};
    p.groups = (unsigned)(p.bricks.bx * p.bricks.by * p.bricks.bz);
    return true;
}

// The launch of a raycast, after the entry's own argument checks: the tiles of the B views and the march.  false: unsupported
// sizes, or more steps than MAX_STEPS.
struct RayPlan {
    RayTiles tiles;
    March march;
    unsigned groups;
};

static inline bool ray_plan(RayPlan& p, int nx, int ny, int nz, int B, int H, int W, float near_disp, float far_disp, float step,
                            int max_steps) {
    if (!sizes_fit(nx, ny, nz, H, W) || max_steps > MAX_STEPS || !ray_tiles_of(p.tiles, B, H, W)) return false;
    p.march = {(double)near_disp, (double)far_disp, (double)step, max_steps};
    p.groups = (unsigned)(p.tiles.per_view * B);
    return true;
}

}  // namespace ecm_vol
