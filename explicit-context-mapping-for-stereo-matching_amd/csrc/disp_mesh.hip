// The mesh of the TSDF volume (include/ecm_mesh.h has the definitions): marching tetrahedra on the Kuhn
// split of every grid cube, as an indexed mesh whose vertices are shared by slot (grid point, one of seven directions) and
// numbered in the order (linear index of the point, direction), with the faces in the order (cube, tetrahedron, triangle).
// The orders are linear, the classification is local in 3-D, so the work is split:
//   count    classify   a workgroup of 256 owns a brick of 16 x 4 x 4 points (x fastest), one thread per point.  The usable and sign
//                       bits of the brick and a halo of one point on every side go into LDS, then the live flags of the cubes
//                       whose low corner lies in the brick or one point below it; a thread forms its point's STATE word -- the
//                       7-bit mask of its slots, the triangles of its cube, the cube's live flag and the signs of its eight
//                       corners -- and writes it to scratch at the point's linear index.
//            tiles      a workgroup owns one linear tile (disp_geom.h) of 2048 points: the vertices and triangles of the tile.
//            scan       ONE workgroup walks the tile counts in chunks of THREADS with a carry: the exclusive scans in place, the
//                       totals into counts[2].
//   emit     vertices   per linear tile: a point's first vertex number is its tile's offset + the counts of the (item, wave)
//                       pairs before its own + the set mask bits of the lanes below it (seven ballots, one per direction); it
//                       goes to scratch (BASE) for the faces, and the point's vertices are written.
//            faces      per linear tile likewise for the triangle counts (four ballots, one per bit); a live cube walks its six
//                       tetrahedra and the table below, and finds the number of a slot (q, dir) as BASE[q] + the set bits of q's
//                       mask below dir -- whichever brick or tile q belongs to.
// No atomics of any kind, no workgroup waits for another (a kernel boundary is the only hand-off), no scratch memory of the
// private kind: the numbering is the linear order whatever the scheduling.  Every store to an output is bounded by the caller's
// capacity and every index into scratch or the volume by the sizes, so a scratch that is not the count pass's gives wrong rows,
// never an access out of bounds.  HBM-bound: 8 B read and 4 B written per point by classify, 4 B read by tiles, vertices and faces
// each, 4 B written by vertices; the surface itself is O(n^2) of the n^3 points.
// The whole file is compiled with contraction off: every product and sum is one IEEE operation, as the header states them.
#include "disp_geom.h"
#include "../../include/ecm_mesh.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using namespace ecm_pix;
constexpr int BX = 16, BY = 4, BZ = 4;                     // points of a brick
constexpr int SX = BX + 2, SY = BY + 2, SZ = BZ + 2;       // staged points: the brick and one point on every side
constexpr int CX = BX + 1, CY = BY + 1, CZ = BZ + 1;       // cubes whose live flag a brick needs: low corner at staged 0 .. B
constexpr long long MAX_POINTS = 1ll << 27;
static_assert(BX * BY * BZ == THREADS, "one thread per point of a brick");

typedef unsigned long long u64;

// the state word of a point
constexpr unsigned MASK = 0x7fu;                           // bit dir: slot (p, dir) carries a vertex
constexpr int NTRI_SHIFT = 7;                              // 4 bits: the triangles of cube p (0 .. 12)
constexpr int NTRI_BITS = 4;
constexpr unsigned LIVE = 1u << 11;                        // cube p is live
constexpr int SIGN_SHIFT = 12;                             // 8 bits: corner x | y << 1 | z << 2 of cube p is positive

// dir 0..6 as x | y << 1 | z << 2: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
__host__ __device__ constexpr int dir_code(int d) { return (0x7653421 >> (4 * d)) & 7; }
// corners c1 and c2 of tetrahedron tet as x | y << 1 | z << 2 (c0 = 0, c3 = 7): the permutations of the axes in lexicographic order
__host__ __device__ constexpr int tet_c1(int tet) { return 1 << (tet >> 1); }
__host__ __device__ constexpr int tet_c2(int tet) { return (0x656353 >> (4 * tet)) & 7; }

__device__ __forceinline__ int tet_case(unsigned signs, int tet) {
    return (int)((signs & 1u) | ((signs >> tet_c1(tet)) & 1u) << 1 | ((signs >> tet_c2(tet)) & 1u) << 2 | ((signs >> 7) & 1u) << 3);
}

// triangles of a case: none where all four corners agree, two where they split two and two, else one
__device__ __forceinline__ int case_triangles(int c) {
    const int n = __popc((unsigned)c);
    return n == 2 ? 2 : (n == 0 || n == 4 ? 0 : 1);
}

// The triangle table, [tet][case][2]: a triangle is three slots of 6 bits each, first slot lowest -- the corner of the cube the
// slot starts at (x | y << 1 | z << 2) and dir << 3 -- and an absent triangle is all ones.  Generated from the rule of
// include/ecm_mesh.h by build_table() of tests/test_volume_mesh_cpu.py, which reads these words back and compares.
static __device__ const unsigned TRI_TABLE[6 * 16 * 2] = {
    0xffffffffu, 0xffffffffu, 0x00018c00u, 0xffffffffu, 0x00029240u, 0xffffffffu, 0x00030a58u, 0x00029258u,
    0x000094d8u, 0xffffffffu, 0x00013c00u, 0x000094c0u, 0x000294c0u, 0x00013600u, 0x000294f0u, 0xffffffffu,
    0x00013a70u, 0xffffffffu, 0x000184c0u, 0x00013a40u, 0x00013240u, 0x000304c0u, 0x00013258u, 0xffffffffu,
    0x00009a58u, 0x00029c18u, 0x00009a40u, 0xffffffffu, 0x00030600u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
    0xffffffffu, 0xffffffffu, 0x00030800u, 0xffffffffu, 0x00011a40u, 0xffffffffu, 0x00029c20u, 0x00011a60u,
    0x0000d460u, 0xffffffffu, 0x00030340u, 0x0000d440u, 0x0000da40u, 0x00020340u, 0x0000da70u, 0xffffffffu,
    0x00029370u, 0xffffffffu, 0x0000d800u, 0x00029340u, 0x00011340u, 0x0000dc00u, 0x00011360u, 0xffffffffu,
    0x00029460u, 0x00030a60u, 0x00029440u, 0xffffffffu, 0x00020c00u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
    0xffffffffu, 0xffffffffu, 0x00030608u, 0xffffffffu, 0x00002888u, 0xffffffffu, 0x00022c18u, 0x00002898u,
    0x00013098u, 0xffffffffu, 0x000304c8u, 0x00013088u, 0x00013888u, 0x000184c8u, 0x000138b0u, 0xffffffffu,
    0x000224f0u, 0xffffffffu, 0x00013608u, 0x000224c8u, 0x000024c8u, 0x00013c08u, 0x000024d8u, 0xffffffffu,
    0x00022098u, 0x00030898u, 0x00022088u, 0xffffffffu, 0x00018c08u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
    0xffffffffu, 0xffffffffu, 0x00028c08u, 0xffffffffu, 0x00022488u, 0xffffffffu, 0x000308a8u, 0x000224a8u,
    0x000121a8u, 0xffffffffu, 0x00006c08u, 0x00012188u, 0x00022188u, 0x00006a08u, 0x000221b0u, 0xffffffffu,
    0x000068b0u, 0xffffffffu, 0x00028188u, 0x00006888u, 0x00006488u, 0x00030188u, 0x000064a8u, 0xffffffffu,
    0x000128a8u, 0x00022c28u, 0x00012888u, 0xffffffffu, 0x00030a08u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
    0xffffffffu, 0xffffffffu, 0x00020c10u, 0xffffffffu, 0x0001c110u, 0xffffffffu, 0x00030720u, 0x0001c120u,
    0x00004360u, 0xffffffffu, 0x0000dc10u, 0x00004350u, 0x0001c350u, 0x0000d810u, 0x0001c370u, 0xffffffffu,
    0x0000d730u, 0xffffffffu, 0x00020350u, 0x0000d710u, 0x0000d110u, 0x00030350u, 0x0000d120u, 0xffffffffu,
    0x00004720u, 0x0001cc20u, 0x00004710u, 0xffffffffu, 0x00030810u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
    0xffffffffu, 0xffffffffu, 0x00030a10u, 0xffffffffu, 0x0000c710u, 0xffffffffu, 0x0001cc28u, 0x0000c728u,
    0x00006328u, 0xffffffffu, 0x00030190u, 0x00006310u, 0x00006710u, 0x00028190u, 0x00006730u, 0xffffffffu,
    0x0001c1b0u, 0xffffffffu, 0x00006a10u, 0x0001c190u, 0x0000c190u, 0x00006c10u, 0x0000c1a8u, 0xffffffffu,
    0x0001c328u, 0x00030728u, 0x0001c310u, 0xffffffffu, 0x00028c10u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
};

// the usable rule of include/ecm_mesh.h: comparisons on input bits only
__device__ __forceinline__ bool usable(float t, float w, float min_weight) { return w > min_weight && ecm_finite(t); }

// lanes of the wave below this one that are set in `ballot`
__device__ __forceinline__ int rank_in_wave(u64 ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// ---- count (a): the state word of every point ------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void mesh_classify(const float* __restrict__ tsdf, const float* __restrict__ wsum,
                                                         unsigned* __restrict__ state, int nx, int ny, int nz, int bx, int by,
                                                         float min_weight) {
    __shared__ unsigned char pt[SZ * SY * SX];                        // bit 0: usable, bit 1: positive; 0 outside the grid
    __shared__ unsigned char lv[CZ * CY * CX];                        // the cube whose low corner is staged point (x, y, z) is live
    const unsigned blk = blockIdx.x;
    const int bi = (int)(blk % (unsigned)bx), bj = (int)((blk / (unsigned)bx) % (unsigned)by), bk = (int)(blk / ((unsigned)bx * (unsigned)by));
    const int x0 = bi * BX - 1, y0 = bj * BY - 1, z0 = bk * BZ - 1;   // the grid point of staged (0, 0, 0)
    for (int idx = threadIdx.x; idx < SX * SY * SZ; idx += THREADS) {
        const int gx = x0 + idx % SX, gy = y0 + (idx / SX) % SY, gz = z0 + idx / (SX * SY);
        unsigned char v = 0;
        if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) {
            const size_t at = ((size_t)gz * ny + gy) * nx + gx;       // below nx * ny * nz <= 2^27
            const float t = tsdf[at];
            v = (unsigned char)((usable(t, wsum[at], min_weight) ? 1 : 0) | (t > 0.f ? 2 : 0));
        }
        pt[idx] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < CX * CY * CZ; idx += THREADS) {
        const int s = ((idx / (CX * CY)) * SY + (idx / CX) % CY) * SX + idx % CX;
        lv[idx] = (unsigned char)(pt[s] & pt[s + 1] & pt[s + SX] & pt[s + SX + 1] & pt[s + SX * SY] & pt[s + SX * SY + 1]
                                  & pt[s + SX * SY + SX] & pt[s + SX * SY + SX + 1] & 1);
    }
    __syncthreads();
    const int tx = threadIdx.x % BX, ty = (threadIdx.x / BX) % BY, tz = threadIdx.x / (BX * BY);
    const int gx = bi * BX + tx, gy = bj * BY + ty, gz = bk * BZ + tz;
    if (gx >= nx || gy >= ny || gz >= nz) return;
    const int sx = tx + 1, sy = ty + 1, sz = tz + 1;
    const int s = (sz * SY + sy) * SX + sx;
    unsigned signs = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) signs |= (unsigned)((pt[s + (((c >> 2) & 1) * SY + ((c >> 1) & 1)) * SX + (c & 1)] >> 1) & 1) << c;
    const bool own = lv[(sz * CY + sy) * CX + sx] != 0;
    int ntri = 0;
    if (own) {
#pragma unroll
        for (int tet = 0; tet < 6; ++tet) ntri += case_triangles(tet_case(signs, tet));
    }
    unsigned mask = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        const int code = dir_code(d), dx = code & 1, dy = (code >> 1) & 1, dz = (code >> 2) & 1;
        const bool differ = ((signs ^ (signs >> code)) & 1u) != 0;   // corner `code` of cube p is the point p + dir
        int any = 0;                                                  // a live cube among those that contain the edge
#pragma unroll
        for (int oz = 0; oz <= 1 - dz; ++oz)
#pragma unroll
            for (int oy = 0; oy <= 1 - dy; ++oy)
#pragma unroll
                for (int ox = 0; ox <= 1 - dx; ++ox) any |= lv[((sz - oz) * CY + (sy - oy)) * CX + (sx - ox)];
        mask |= (differ && any) ? 1u << d : 0u;
    }
    state[((size_t)gz * ny + gy) * nx + gx] = mask | (unsigned)ntri << NTRI_SHIFT | (own ? LIVE : 0u) | signs << SIGN_SHIFT;
}

// ---- count (b): the vertices and triangles of each linear tile -------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void mesh_tile_count(const unsigned* __restrict__ state, int* __restrict__ tile_v,
                                                           int* __restrict__ tile_f, unsigned P) {
    __shared__ int per_wave[2 * NWAVE];
    const unsigned first = blockIdx.x * (unsigned)TILE;
    int nv = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned p = first + k * THREADS + threadIdx.x;
        const unsigned s = p < P ? state[p] : 0u;
        nv += __popc(s & MASK);
        nf += (int)((s >> NTRI_SHIFT) & ((1u << NTRI_BITS) - 1));
    }
    nv = wave_sum(nv);
    nf = wave_sum(nf);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        per_wave[threadIdx.x / WAVE] = nv;
        per_wave[NWAVE + threadIdx.x / WAVE] = nf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sv = 0, sf = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) sv += per_wave[w], sf += per_wave[NWAVE + w];
        tile_v[blockIdx.x] = sv;
        tile_f[blockIdx.x] = sf;
    }
}

// ---- count (c): the exclusive scans of the T tile counts, in place, by one workgroup; the totals -----------------------------------
__global__ __launch_bounds__(THREADS) void mesh_scan(int* __restrict__ tile_v, int* __restrict__ tile_f, long long* __restrict__ counts, int T) {
    __shared__ int per_wave[2 * NWAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int carry_v = 0, carry_f = 0;                                     // at most 7 * 2^27 and 12 * 2^27: below 2^31
    for (int base = 0; base < T; base += THREADS) {
        const int i = base + threadIdx.x;
        const int v = i < T ? tile_v[i] : 0, f = i < T ? tile_f[i] : 0;
        int sv = v, sf = f;                                           // inclusive scans within the wave
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int uv = __shfl_up(sv, off, WAVE), uf = __shfl_up(sf, off, WAVE);
            if (lane >= off) sv += uv, sf += uf;
        }
        if (lane == WAVE - 1) per_wave[wave] = sv, per_wave[NWAVE + wave] = sf;
        __syncthreads();
        int before_v = 0, total_v = 0, before_f = 0, total_f = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            const int cv = per_wave[w], cf = per_wave[NWAVE + w];
            before_v += w < wave ? cv : 0, total_v += cv;
            before_f += w < wave ? cf : 0, total_f += cf;
        }
        if (i < T) {
            tile_v[i] = carry_v + before_v + sv - v;
            tile_f[i] = carry_f + before_f + sf - f;
        }
        carry_v += total_v, carry_f += total_f;
        __syncthreads();                                              // per_wave is rewritten by the next chunk
    }
    if (threadIdx.x == 0) counts[0] = carry_v, counts[1] = carry_f;
}

// ---- emit (a): every point's first vertex number, and the vertices ---------------------------------------------------------------
struct Grid {
    int nx, ny, nz;
    unsigned P;
};

// the header's gradient along one axis at the point `at` (coordinate c of n along the axis, `stride` elements apart)
__device__ __forceinline__ double gradient_axis(const float* __restrict__ tsdf, const float* __restrict__ wsum, size_t at, int c, int n,
                                                size_t stride, float min_weight) {
    const double t = (double)tsdf[at];
    double hi = 0.0, lo = 0.0;
    bool has_hi = false, has_lo = false;
    if (c + 1 < n) {
        const float v = tsdf[at + stride];
        has_hi = usable(v, wsum[at + stride], min_weight);
        hi = (double)v;
    }
    if (c >= 1) {
        const float v = tsdf[at - stride];
        has_lo = usable(v, wsum[at - stride], min_weight);
        lo = (double)v;
    }
    return has_hi && has_lo ? hi - lo : (has_hi ? hi - t : (has_lo ? t - lo : 0.0));
}

__global__ __launch_bounds__(THREADS) void mesh_vertices(const float* __restrict__ tsdf, const float* __restrict__ wsum,
                                                         const double* __restrict__ M, const unsigned* __restrict__ state,
                                                         const int* __restrict__ tile_v, int* __restrict__ base,
                                                         float* __restrict__ vertices, float* __restrict__ normals,
                                                         float* __restrict__ weight, long long capacity, Grid g, float min_weight) {
    __shared__ __align__(16) int count[ITEMS * NWAVE];                // [item][wave]
    static_assert(NWAVE == 4, "an item's counts are read as one int4");
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const unsigned first = blockIdx.x * (unsigned)TILE;
    unsigned masks = 0;                                               // 7 bits per item: ITEMS * 7 = 56 bits, in two words
    unsigned masks_hi = 0;
    int below[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned p = first + k * THREADS + threadIdx.x;
        const unsigned m = p < g.P ? state[p] & MASK : 0u;
        int b = 0, total = 0;
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            const u64 ballot = __ballot((m >> d) & 1u);
            b += rank_in_wave(ballot);
            total += __popcll(ballot);
        }
        below[k] = b;
        if (k < 4) masks |= m << (7 * k); else masks_hi |= m << (7 * (k - 4));
        if (lane == 0) count[k * NWAVE + wave] = total;
    }
    __syncthreads();

    int run = tile_v[blockIdx.x];                                     // vertices before item k of this tile
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
#pragma unroll 1
    for (int k = 0; k < ITEMS; ++k) {
        const int4 c = reinterpret_cast<const int4*>(count)[k];
        const int before = run + (wave > 0 ? c.x : 0) + (wave > 1 ? c.y : 0) + (wave > 2 ? c.z : 0);
        run += c.x + c.y + c.z + c.w;
        const unsigned p = first + k * THREADS + threadIdx.x;
        if (p >= g.P) continue;
        int b = 0;                                                    // below[k] without a dynamic index into registers
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) b = j == k ? below[j] : b;
        long long row = (long long)before + b;
        base[p] = (int)row;
        unsigned m = ((k < 4 ? masks >> (7 * k) : masks_hi >> (7 * (k - 4)))) & MASK;
        if (!m) continue;
        const int z = (int)(p / (unsigned)sz), y = (int)((p - (unsigned)z * (unsigned)sz) / (unsigned)g.nx);
        const int x = (int)(p - (unsigned)z * (unsigned)sz - (unsigned)y * (unsigned)g.nx);
        const double t0 = (double)tsdf[p];
        double G0x = 0.0, G0y = 0.0, G0z = 0.0;
        if (normals) {
            G0x = gradient_axis(tsdf, wsum, p, x, g.nx, 1, min_weight);
            G0y = gradient_axis(tsdf, wsum, p, y, g.ny, sy, min_weight);
            G0z = gradient_axis(tsdf, wsum, p, z, g.nz, sz, min_weight);
        }
        for (; m; m &= m - 1, ++row) {
            const int d = __ffs((int)m) - 1, code = dir_code(d);
            const int dx = code & 1, dy = (code >> 1) & 1, dz = (code >> 2) & 1;
            if (row < 0 || row >= capacity) continue;                 // the rows that fit are written
            if (x + dx >= g.nx || y + dy >= g.ny || z + dz >= g.nz) continue;   // never with the count pass's own scratch
            const size_t q = (size_t)p + dx + dy * sy + dz * sz;
            const double t1 = (double)tsdf[q];
            const double a = t0 / (t0 - t1);
            const double gx = (double)x + (double)dx * a, gy = (double)y + (double)dy * a, gz = (double)z + (double)dz * a;
            float* v = vertices + 3 * (size_t)row;
            v[0] = (float)ecm_row4(M, gx, gy, gz);
            v[1] = (float)ecm_row4(M + 4, gx, gy, gz);
            v[2] = (float)ecm_row4(M + 8, gx, gy, gz);
            if (normals) {
                const double G1x = gradient_axis(tsdf, wsum, q, x + dx, g.nx, 1, min_weight);
                const double G1y = gradient_axis(tsdf, wsum, q, y + dy, g.ny, sy, min_weight);
                const double G1z = gradient_axis(tsdf, wsum, q, z + dz, g.nz, sz, min_weight);
                const double n0 = G0x + a * (G1x - G0x), n1 = G0y + a * (G1y - G0y), n2 = G0z + a * (G1z - G0z);
                const double m0 = (M[0] * n0 + M[1] * n1) + M[2] * n2, m1 = (M[4] * n0 + M[5] * n1) + M[6] * n2;
                const double m2 = (M[8] * n0 + M[9] * n1) + M[10] * n2;
                const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
                const bool ok = ecm_finite(len) && len != 0.0;
                float* n = normals + 3 * (size_t)row;
                n[0] = ok ? (float)(m0 / len) : 0.f;
                n[1] = ok ? (float)(m1 / len) : 0.f;
                n[2] = ok ? (float)(m2 / len) : 0.f;
            }
            if (weight) {
                const double w0 = (double)wsum[p], w1 = (double)wsum[q];
                weight[row] = (float)(w0 + a * (w1 - w0));
            }
        }
    }
}

// ---- emit (b): the faces -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void mesh_faces(const unsigned* __restrict__ state, const int* __restrict__ tile_f,
                                                      const int* __restrict__ base, int* __restrict__ faces, long long capacity, Grid g) {
    __shared__ __align__(16) int count[ITEMS * NWAVE];                // [item][wave]
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const unsigned first = blockIdx.x * (unsigned)TILE;
    unsigned live_bits = 0;                                           // bit k: item k is a live cube with triangles
    int below[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned p = first + k * THREADS + threadIdx.x;
        const unsigned s = p < g.P ? state[p] : 0u;
        const unsigned n = (s >> NTRI_SHIFT) & ((1u << NTRI_BITS) - 1);
        int b = 0, total = 0;
#pragma unroll
        for (int bit = 0; bit < NTRI_BITS; ++bit) {
            const u64 ballot = __ballot((n >> bit) & 1u);
            b += rank_in_wave(ballot) << bit;
            total += __popcll(ballot) << bit;
        }
        below[k] = b;
        live_bits |= (n != 0 && (s & LIVE)) ? 1u << k : 0u;
        if (lane == 0) count[k * NWAVE + wave] = total;
    }
    __syncthreads();

    int run = tile_f[blockIdx.x];                                     // triangles before item k of this tile
    const unsigned sy = (unsigned)g.nx, sz = (unsigned)g.nx * (unsigned)g.ny;
#pragma unroll 1
    for (int k = 0; k < ITEMS; ++k) {
        const int4 c = reinterpret_cast<const int4*>(count)[k];
        const int before = run + (wave > 0 ? c.x : 0) + (wave > 1 ? c.y : 0) + (wave > 2 ? c.z : 0);
        run += c.x + c.y + c.z + c.w;
        if (!((live_bits >> k) & 1u)) continue;
        const unsigned p = first + k * THREADS + threadIdx.x;         // below P: the state was read
        int b = 0;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) b = j == k ? below[j] : b;
        long long row = (long long)before + b;
        const unsigned signs = (state[p] >> SIGN_SHIFT) & 0xffu;
#pragma unroll 1
        for (int tet = 0; tet < 6; ++tet) {
            const int cs = tet_case(signs, tet);
#pragma unroll 1
            for (int tri = 0; tri < 2; ++tri) {
                const unsigned e = TRI_TABLE[(tet * 16 + cs) * 2 + tri];
                if (e == 0xffffffffu) break;
                int id[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const unsigned ref = (e >> (6 * j)) & 63u, corner = ref & 7u, dir = ref >> 3;
                    const unsigned q = p + (corner & 1u) + ((corner >> 1) & 1u) * sy + (corner >> 2) * sz;
                    id[j] = q < g.P ? base[q] + __popc(state[q] & ((1u << dir) - 1u)) : 0;   // q >= P: never with the count pass's own scratch
                }
                if (row >= 0 && row < capacity) {
                    int* f = faces + 3 * (size_t)row;
                    f[0] = id[0], f[1] = id[1], f[2] = id[2];
                }
                ++row;
            }
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Plan {
    long long P;
    int T;
    int bx, by, bz;
};

// the sizes both entries are built for; code: why not
bool plan_of(int nx, int ny, int nz, Plan& plan, int& code) {
    code = ECM_EINVAL;
    if (nx < 2 || ny < 2 || nz < 2) return false;
    code = ECM_EUNSUP;
    if ((long long)nx * ny > MAX_POINTS || (long long)nx * ny * nz > MAX_POINTS) return false;   // after dims >= 2: no overflow
    plan.P = (long long)nx * ny * nz;
    plan.T = ecm_pix_tiles(plan.P, 1, code);
    if (!plan.T) return false;
    plan.bx = (nx + BX - 1) / BX, plan.by = (ny + BY - 1) / BY, plan.bz = (nz + BZ - 1) / BZ;   // at most 2^27 / 4 bricks
    code = 0;
    return true;
}

long long bytes_of(const Plan& plan) { return ((2 * plan.P + 2 * (long long)plan.T) * 4 + 15) / 16 * 16; }

struct Scratch {
    unsigned* state;                          // [P]
    int* base;                                // [P]
    int* tile_v;                              // [T]
    int* tile_f;                              // [T]
};

Scratch carve(void* scratch, const Plan& plan) {
    Scratch s;
    s.state = static_cast<unsigned*>(scratch);
    s.base = reinterpret_cast<int*>(s.state + plan.P);
    s.tile_v = s.base + plan.P;
    s.tile_f = s.tile_v + plan.T;
    return s;
}

bool weight_ok(float min_weight) { return std::isfinite(min_weight) && min_weight >= 0.f; }

}  // namespace

extern "C" int ecms_mesh_tile(void) { return TILE; }

extern "C" int ecms_mesh_brick(int axis) { return axis == 0 ? BX : (axis == 1 ? BY : (axis == 2 ? BZ : 0)); }

extern "C" long long ecms_mesh_scratch_bytes(int nx, int ny, int nz) {
    Plan plan;
    int code;
    return plan_of(nx, ny, nz, plan, code) ? bytes_of(plan) : 0;
}

extern "C" int ecms_mesh_count_fwd(const float* tsdf, const float* wsum, long long* counts, void* scratch, long long scratch_bytes,
                                   int nx, int ny, int nz, float min_weight, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && counts && scratch);
    ECM_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2 && weight_ok(min_weight));
    ECM_CHECK_ARG(ecm_no_alias({counts, scratch}, {tsdf, wsum}) && (const void*)counts != scratch);
    Plan plan;
    int code;
    if (!plan_of(nx, ny, nz, plan, code)) return code;
    ECM_CHECK_ARG(scratch_bytes >= bytes_of(plan));
    const Scratch s = carve(scratch, plan);
    hipStream_t st = ecm_stream(stream);
    hipLaunchKernelGGL(mesh_classify, dim3((unsigned)(plan.bx * plan.by * plan.bz)), dim3(THREADS), 0, st, tsdf, wsum, s.state, nx, ny, nz,
                       plan.bx, plan.by, min_weight);
    hipLaunchKernelGGL(mesh_tile_count, dim3((unsigned)plan.T), dim3(THREADS), 0, st, (const unsigned*)s.state, s.tile_v, s.tile_f,
                       (unsigned)plan.P);
    hipLaunchKernelGGL(mesh_scan, dim3(1), dim3(THREADS), 0, st, s.tile_v, s.tile_f, counts, plan.T);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecms_mesh_emit_fwd(const float* tsdf, const float* wsum, const double* M, float* vertices, int* faces, float* normals,
                                  float* weight, void* scratch, long long scratch_bytes, long long n_vertices, long long n_faces, int nx,
                                  int ny, int nz, float min_weight, void* stream) {
    ECM_CHECK_ARG(tsdf && wsum && M && vertices && faces && scratch);
    ECM_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2 && weight_ok(min_weight) && n_vertices >= 0 && n_faces >= 0);
    ECM_CHECK_ARG(ecm_no_alias({vertices, faces, normals, weight, scratch}, {tsdf, wsum, M}));
    const void* outs[5] = {vertices, faces, normals, weight, scratch};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) ECM_CHECK_ARG(!outs[i] || outs[i] != outs[j]);
    Plan plan;
    int code;
    if (!plan_of(nx, ny, nz, plan, code)) return code;
    ECM_CHECK_ARG(scratch_bytes >= bytes_of(plan));
    const Scratch s = carve(scratch, plan);
    const Grid g = {nx, ny, nz, (unsigned)plan.P};
    hipStream_t st = ecm_stream(stream);
    hipLaunchKernelGGL(mesh_vertices, dim3((unsigned)plan.T), dim3(THREADS), 0, st, tsdf, wsum, M, (const unsigned*)s.state,
                       (const int*)s.tile_v, s.base, vertices, normals, weight, n_vertices, g, min_weight);
    hipLaunchKernelGGL(mesh_faces, dim3((unsigned)plan.T), dim3(THREADS), 0, st, (const unsigned*)s.state, (const int*)s.tile_f,
                       (const int*)s.base, faces, n_faces, g);
    return ECM_LAUNCH_RESULT();
}
