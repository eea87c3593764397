// The speckle filter of a disparity map (include/ecm_hip.h has the definitions): the connected segments of
// the graph "4-neighbours, both usable, |d[p] - d[q]| <= max_diff", each pixel's segment label (the row-major index of the
// segment's first pixel) and size, and d with the segments of at most max_size pixels set to 0.  Connected-component labelling
// by union-find over int32 parents, four launches on the one stream:
//   local    a workgroup of 256 threads owns a tile of TW x TH pixels at a time (a wave is 64 consecutive x of one row and takes
//            the rows wave, wave + 4) and walks tiles GRID apart.  It stages d into LDS (NaN where not usable, as disp_filter.hip
//            does), starts every pixel at the first pixel of its horizontal run (one ballot per row), unites the runs of
//            neighbouring rows in LDS, and writes each pixel's parent -- its tile's root, as an index into the image -- into
//            `label` and, at a root, the pixel count of the tile's part of the segment into `size` (0 elsewhere);
//   merge    one thread per pair of 4-neighbours that a tile border separates: a union on the parents in `label`;
//   count    each pixel walks to its root and parks it in its own slot of `out`; a tile's root that is not the segment's root adds
//            its count to the root's;
//   emit     each pixel reads the size at its root and writes label, size and out.
// Termination does not depend on scheduling: a parent is never larger than its child, so every step of a `find` and every retry
// of a `unite` strictly decreases a non-negative integer; no workgroup waits for another, there is no loop on a flag.  Integer
// atomics only (min on parents, add on counts), no inline assembly, no private segment, no scratch buffer.
#include "disp_geom.h"

namespace {

constexpr int THREADS = 256, WAVE = 64, NWAVE = THREADS / WAVE;
constexpr int TW = 64, TH = 8;                // the tile: a wave is one row of it, and takes TH / NWAVE rows
constexpr int ROWS = TH / NWAVE;              // rows of a tile per wave
constexpr int GRID = 1024;                    // workgroups of a launch (four per CU); each walks its work GRID apart

// ---- union-find over parents with parent <= child ------------------------------------------------------------------------------
// SCOPE is the memory scope of the parents: the workgroup for a tile's forest in LDS, the agent for the image's forest in global
// memory during `merge`, where other workgroups -- on other XCDs, behind other L2s -- unite at the same time.  A read may return
// any value the parent has held: parents only ever decrease (the one write is a min), and every value one has held is a member of
// the same segment and an ancestor, so a stale read makes the walk end at a node that has stopped being a root, never at a node
// of another segment.  The min then returns something other than that node, and the union is tried again from what it returned.
template <int SCOPE>
__device__ __forceinline__ int find_root(int* parent, int i) {
    for (;;) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, SCOPE);
        if (p == i) return i;                                               // p < i otherwise: the walk descends
        i = p;
    }
}

template <int SCOPE>
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root<SCOPE>(parent, a);
        b = find_root<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);      // b < a
        if (old == a) return;                                               // a was a root and hangs under b now
        a = old;                                                            // old < a: a had a parent already; unite that with b.
    }                                                                       // max(a, b) has decreased: the loop ends
}

// the tile walk and the samples (NaN where not usable: then every comparison is false) are disp_geom.h's
__device__ __forceinline__ bool joined(float a, float b, float max_diff) { return fabsf(a - b) <= max_diff; }

// ---- local: the segments of each tile ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void speckle_local(const float* __restrict__ d, const unsigned char* __restrict__ valid,
                                                         int* __restrict__ label, int* __restrict__ size, int B, int H, int W,
                                                         float max_diff) {
    __shared__ float D[TH * TW];              // the tile, NaN where not usable (outside the image too)
    __shared__ int P[TH * TW];                // parents, as indices into the tile
    __shared__ int N[TH * TW];                // pixel counts, at the roots
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const Tiles2D t = ecm_tiles_of<TW, TH>(B, H, W);
    const size_t image = (size_t)H * W;

    for (long long tile = blockIdx.x; tile < t.n; tile += gridDim.x) {
        const int b = (int)(tile / ((long long)t.tx * t.ty));
        const int rest = (int)(tile - (long long)b * t.tx * t.ty);
        const int y0 = (rest / t.tx) * TH, x0 = (rest % t.tx) * TW;
        const int x = x0 + lane;
        float v[ROWS];
        bool left[ROWS];                      // joined with the pixel on its left, inside the tile
        int root[ROWS];

        // stage; a pixel starts at the first pixel of its run of left-joined pixels, so the horizontal edges are done
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int ty = wave + k * NWAVE, y = y0 + ty, i = ty * TW + lane;
            v[k] = __builtin_nanf("");
            if (y < H && x < W) v[k] = ecm_disp_or_nan(d, valid, b * image + (size_t)y * W + x);
            const float vl = __shfl_up(v[k], 1, WAVE);
            left[k] = lane > 0 && joined(v[k], vl, max_diff);
            const bool usable = v[k] == v[k];
            const unsigned long long starts = __ballot(usable && !left[k]);               // lanes at which a run starts
            const int start = 63 - __builtin_clzll((starts & (~0ull >> (63 - lane))) | 1ull);   // the nearest at or below this lane
            D[i] = v[k];
            P[i] = usable ? ty * TW + start : -1;
            N[i] = 0;
        }
        __syncthreads();

        // the vertical edges.  One that closes a square of three joined edges -- the left neighbours of both ends are joined to
        // them and to each other -- is implied by those three and left out: a constant tile takes TH - 1 unions, not TH * TW
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int ty = wave + k * NWAVE, i = ty * TW + lane;
            if (ty > 0) {                                                   // wave-uniform
                const float vu = D[i - TW];
                const bool up = joined(v[k], vu, max_diff);
                const bool left_up = lane > 0 && joined(vu, D[i - TW - (lane > 0 ? 1 : 0)], max_diff);
                const bool up_left = __shfl_up((int)up, 1, WAVE) != 0;
                if (up && !(left[k] && left_up && up_left)) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(P, i, i - TW);
            }
        }
        __syncthreads();

        // every pixel to its root; the roots count
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int i = (wave + k * NWAVE) * TW + lane;
            root[k] = -1;
            if (v[k] == v[k]) {
                root[k] = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(P, i);
                atomicAdd(&N[root[k]], 1);
            }
        }
        __syncthreads();

#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int ty = wave + k * NWAVE, y = y0 + ty, i = ty * TW + lane;
            if (y < H && x < W) {
                const size_t at = b * image + (size_t)y * W + x;
                const int r = root[k];
                label[at] = r < 0 ? -1 : (y0 + r / TW) * W + x0 + r % TW;      // the root as an index into the image
                size[at] = r == i ? N[i] : 0;
            }
        }
        __syncthreads();                                                    // the next tile overwrites D, P and N
    }
}

// ---- merge: the edges that cross a tile border ---------------------------------------------------------------------------------
// Per image (ty - 1) W pairs across the horizontal borders, then (tx - 1) H pairs across the vertical ones, one thread each.  An
// edge that closes a square whose other three edges are joined is left out, as above, but only where two of those three lie
// inside tiles (done by `local`) and the third is the same border's previous pair: no edge is left out on the strength of
// another that is left out on the strength of it.  The parents are read and written here by agent-scope atomics only.
__global__ __launch_bounds__(THREADS) void speckle_merge(const float* __restrict__ d, const unsigned char* __restrict__ valid,
                                                         int* label, int B, int H, int W, float max_diff) {
    const Tiles2D t = ecm_tiles_of<TW, TH>(B, H, W);
    const size_t image = (size_t)H * W;
    const long long across = (long long)(t.ty - 1) * W, per = across + (long long)(t.tx - 1) * H, total = per * B;
    for (long long e = (long long)blockIdx.x * THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * THREADS) {
        const int b = (int)(e / per);
        const long long r = e - (long long)b * per;
        int x, y, back;                       // the pixel, and the distance to its partner on the other side of the border
        bool inner;                           // the pair has a previous pair along the same border inside the same two tiles
        if (r < across) {
            y = ((int)(r / W) + 1) * TH, x = (int)(r % W), back = W;
            inner = x % TW != 0;
        } else {
            const long long q = r - across;
            x = ((int)(q / H) + 1) * TW, y = (int)(q % H), back = 1;
            inner = y % TH != 0;
        }
        const float* di = d + b * image;
        const unsigned char* vi = valid ? valid + b * image : nullptr;
        const int p = y * W + x, q = p - back;
        const float vp = ecm_disp_or_nan(di, vi, p), vq = ecm_disp_or_nan(di, vi, q);
        if (!joined(vp, vq, max_diff)) continue;
        if (inner) {
            const int side = back == W ? 1 : W;                             // to the previous pair along the border
            const float vps = ecm_disp_or_nan(di, vi, p - side), vqs = ecm_disp_or_nan(di, vi, q - side);
            if (joined(vp, vps, max_diff) && joined(vq, vqs, max_diff) && joined(vps, vqs, max_diff)) continue;
        }
        unite<__HIP_MEMORY_SCOPE_AGENT>(label + b * image, p, q);
    }
}

// ---- count: every pixel's root, and the segments' sizes ------------------------------------------------------------------------
// Nothing writes `label` here, so plain loads.  `out` holds the root until `emit` (the bits of an int; -1: not usable).  A pixel
// that was its tile's root (its count is not 0) and is not the segment's adds its count to the segment's root: nobody adds to the
// slot it reads (adds go to segment roots only), and a segment's root neither reads nor writes its own slot.
__global__ __launch_bounds__(THREADS) void speckle_count(const int* __restrict__ label, int* size, int* __restrict__ parked, int n,
                                                         int image) {
    for (long long e = (long long)blockIdx.x * THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * THREADS) {
        const int i = (int)e, base = i / image * image, first = label[i];
        int root = first;
        if (first >= 0)
            for (int p = label[base + root]; p != root; p = label[base + root]) root = p;
        parked[i] = root;
        if (root >= 0 && root != i - base) {
            const int mine = size[i];                                       // not 0: i was its tile's root
            if (mine) atomicAdd(size + base + root, mine);
        }
    }
}

// ---- emit -------------------------------------------------------------------------------------------------------------------------
// Only the slots of segment roots are read from `size`, and a root does not write its own: race-free in place.
// `out` is passed as the ints that `count` parked in it, and written as the bits of the result.
__global__ __launch_bounds__(THREADS) void speckle_emit(const float* __restrict__ d, int* __restrict__ out, int* __restrict__ label,
                                                        int* size, int n, int image, int max_size) {
    for (long long e = (long long)blockIdx.x * THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * THREADS) {
        const int i = (int)e, base = i / image * image, root = out[i];
        float o = 0.f;
        if (root >= 0) {
            const int s = size[base + root];
            label[i] = root;
            if (i - base != root) size[i] = s;
            if (s > max_size) o = d[i];
        }
        out[i] = __float_as_int(o);
    }
}

inline int grid_for(long long items) {
    const long long n = (items + THREADS - 1) / THREADS;
    return (int)(n < GRID ? n : GRID);
}

}  // namespace

extern "C" int ecm_disp_speckle_fwd(const float* d, const unsigned char* valid, float* out, int* segments, int B, int H, int W,
                                    int max_size, float max_diff, void* stream) {
    ECM_CHECK_ARG(d && out && segments && B > 0 && H > 0 && W > 0 && max_size >= 0 && max_diff >= 0.f &&
                  max_diff < __builtin_inff());
    if ((long long)B * H * W > INT_MAX) return ECM_EUNSUP;
    const Tiles2D t = ecm_tiles_of<TW, TH>(B, H, W);
    const int image = H * W, n = B * image;
    int* label = segments;
    int* size = segments + n;
    const long long pairs = ((long long)(t.ty - 1) * W + (long long)(t.tx - 1) * H) * B;
    const dim3 block(THREADS);
    hipStream_t s = ecm_stream(stream);
    hipLaunchKernelGGL(speckle_local, dim3((int)(t.n < GRID ? t.n : GRID)), block, 0, s, d, valid, label, size, B, H, W, max_diff);
    if (pairs > 0) hipLaunchKernelGGL(speckle_merge, dim3(grid_for(pairs)), block, 0, s, d, valid, label, B, H, W, max_diff);
    hipLaunchKernelGGL(speckle_count, dim3(grid_for(n)), block, 0, s, label, size, reinterpret_cast<int*>(out), n, image);
    hipLaunchKernelGGL(speckle_emit, dim3(grid_for(n)), block, 0, s, d, reinterpret_cast<int*>(out), label, size, n, image, max_size);
    return ECM_LAUNCH_RESULT();
}
