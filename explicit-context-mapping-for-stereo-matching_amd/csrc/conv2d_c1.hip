// The cmf decoder's output layer, Conv2d(Ci -> 1, 3x3, pad 1, bias) + ReLU (super_resolution_refinement.conv_out + crap,
// cmf.py:259-264) at full resolution: forward, data gradient, weight + bias gradient; and the per-channel sum that is the bias
// gradient of the decoder's ConvTranspose2d layers.
// With ONE output channel the implicit GEMM of the 2-D family would waste 31/32 of every MFMA; the layer is bound by reading the
// Ci input planes (forward, weight gradient) or writing them (data gradient), so all three are plain vector-ALU kernels in the
// manner of conv3d_c1.hip: a workgroup owns a 64 x 32 tile of output pixels, every thread 4 x 2 of them, and the input halo of
// a chunk of C1_CC channels is staged in LDS; the weights are wave-uniform (scalar loads).
// Every reduction has a fixed order (per-thread sums, a fixed shuffle tree, the four waves in order, then the tiles in order):
// the gradients are bit-reproducible, and no float atomics are used.
#include "common.h"

namespace {

constexpr int C1_TX = 64, C1_TY = 32;                    // output tile
constexpr int C1_HX = C1_TX + 2, C1_HY = C1_TY + 2;      // halo tile (pad 1)
constexpr int C1_RS = 68;                                // LDS row stride
constexpr int C1_PLANE = C1_HY * C1_RS;
constexpr int C1_CC = 4;                                 // channels staged per step
constexpr int C1_SUB = 4;                                // weight gradient: tiles (down the image) per workgroup
constexpr int C1_HPOS = C1_HY * C1_HX;                   // 2244 halo positions per channel

// Stage channels [c0, c0 + C1_CC) of image xb (zero outside the image and for channels >= Ci) into Xs[cc][hy][C1_RS].
__device__ __forceinline__ void c1_stage(float* Xs, const float* __restrict__ xb, int c0, int Ci, int H, int W, int y0, int x0) {
    const size_t HW = (size_t)H * W;
    for (int e = threadIdx.x; e < C1_CC * C1_HPOS; e += 256) {
        const int cc = e / C1_HPOS, p = e - cc * C1_HPOS;
        const int hy = p / C1_HX, hx = p - hy * C1_HX;
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx, c = c0 + cc;
        float v = 0.f;
        if (c < Ci && gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(size_t)c * HW + (size_t)gy * W + gx];
        Xs[cc * C1_PLANE + hy * C1_RS + hx] = v;
    }
}

// relu mask of the forward output applied to the incoming gradient: g = gy * (y > 0) (torch's threshold_backward on the result)
__device__ __forceinline__ float c1_g(const float* __restrict__ gy, const float* __restrict__ y, size_t i) {
    return y[i] > 0.f ? gy[i] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// y[b,0,p] = relu(bias + sum_{ci,ky,kx} w[ci,ky,kx] x[b,ci,p + (ky-1, kx-1)])
__global__ __launch_bounds__(256) void conv2d_c1_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ y, int Ci, int H,
                                                     int W, int tiles_x, int tiles_y) {
    __shared__ float Xs[C1_CC * C1_PLANE];
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int y0 = ty * C1_TY, x0 = tx * C1_TX;
    const int lx = (threadIdx.x & 15) * 4, ly = (threadIdx.x >> 4) * 2;
    const float* xb = x + (size_t)b * Ci * H * W;
    float acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
    for (int c0 = 0; c0 < Ci; c0 += C1_CC) {
        __syncthreads();
        c1_stage(Xs, xb, c0, Ci, H, W, y0, x0);
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < C1_CC; ++cc) {
            const int c = c0 + cc;
            if (c >= Ci) break;
            float win[4][6];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 6; ++j) win[r][j] = Xs[cc * C1_PLANE + (ly + r) * C1_RS + lx + j];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float wv = w[c * 9 + ky * 3 + kx];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[r][j] = fmaf(wv, win[r + ky][j + kx], acc[r][j]);
                }
        }
    }
    const float bv = bias[0];
    float* yb = y + (size_t)b * H * W;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int gy = y0 + ly + r, gx = x0 + lx;
        if (gy >= H) continue;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaxf(acc[r][j] + bv, 0.f);
        float* p = yb + (size_t)gy * W + gx;
        if (gx + 4 <= W && (reinterpret_cast<size_t>(p) & 15) == 0) {
            *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (gx + j < W) p[j] = o[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- data gradient
// gx[b,ci,p] = sum_{ky,kx} w[ci,ky,kx] g[b, p - (ky-1, kx-1)],  g = gy * (y > 0).  The masked gradient's halo is staged once;
// each thread keeps its 4 x 6 window in registers and writes its 4 x 2 pixels of every channel.
__global__ __launch_bounds__(256) void conv2d_c1_dgrad(const float* __restrict__ gy, const float* __restrict__ y,
                                                       const float* __restrict__ w, float* __restrict__ gx, int Ci, int H,
                                                       int W, int tiles_x, int tiles_y) {
    __shared__ float Gs[C1_PLANE];
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int y0 = ty * C1_TY, x0 = tx * C1_TX;
    const int lx = (threadIdx.x & 15) * 4, ly = (threadIdx.x >> 4) * 2;
    const size_t HW = (size_t)H * W;
    const float* gyb = gy + (size_t)b * HW;
    const float* yb = y + (size_t)b * HW;
    for (int p = threadIdx.x; p < C1_HPOS; p += 256) {
        const int hy = p / C1_HX, hx = p - hy * C1_HX;
        const int sy = y0 - 1 + hy, sx = x0 - 1 + hx;
        Gs[hy * C1_RS + hx] = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? c1_g(gyb, yb, (size_t)sy * W + sx) : 0.f;
    }
    __syncthreads();
    float win[4][6];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 6; ++j) win[r][j] = Gs[(ly + r) * C1_RS + lx + j];
    float* gxb = gx + (size_t)b * Ci * HW;
    const bool vec = x0 + lx + 4 <= W && (W & 3) == 0 && (reinterpret_cast<size_t>(gx) & 15) == 0;
    for (int c = 0; c < Ci; ++c) {
        float o[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[r][j] = 0.f;
        // output pixel (ly + r, lx + j) reads g at (ly + r + 1 - ky, lx + j + 1 - kx) = win[r + 2 - ky][j + 2 - kx]
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float wv = w[c * 9 + ky * 3 + kx];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[r][j] = fmaf(wv, win[r + 2 - ky][j + 2 - kx], o[r][j]);
            }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int py = y0 + ly + r, px = x0 + lx;
            if (py >= H) continue;
            float* p = gxb + (size_t)c * HW + (size_t)py * W + px;
            if (vec) {
                *reinterpret_cast<float4*>(p) = make_float4(o[r][0], o[r][1], o[r][2], o[r][3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < W) p[j] = o[r][j];
            }
        }
    }
}

// -------------------------------------------------------------------------------------------- weight and bias gradient
// Workgroup = a column of C1_SUB tiles of one image.  partial[wg][ci*9 + k] = sum over its pixels p of x[ci, p + k'] g[p];
// partial[wg][Ci*9] = sum g.  A thread's 8 masked gradient values per tile stay in registers for the whole channel loop.
__device__ __forceinline__ float c1_block_sum_to(float v, float* red, int slot) {
    v = wave_sum(v);                                     // fixed shuffle tree
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 40 + slot] = v;
    return v;
}

__global__ __launch_bounds__(256) void conv2d_c1_wgrad(const float* __restrict__ x, const float* __restrict__ gy,
                                                       const float* __restrict__ y, float* __restrict__ partial, int Ci,
                                                       int H, int W, int tiles_x, int strips_y) {
    __shared__ float Xs[C1_CC * C1_PLANE];
    __shared__ float red[4 * 40];
    const int n = Ci * 9 + 1;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int sy = bid % strips_y;
    const int b = bid / strips_y;
    const int x0 = tx * C1_TX;
    const int lx = (threadIdx.x & 15) * 4, ly = (threadIdx.x >> 4) * 2;
    const size_t HW = (size_t)H * W;
    const float* xb = x + (size_t)b * Ci * HW;
    float g[C1_SUB][2][4];
    float gsum = 0.f;
#pragma unroll
    for (int s = 0; s < C1_SUB; ++s)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int py = (sy * C1_SUB + s) * C1_TY + ly + r, px = x0 + lx + j;
                g[s][r][j] = (py < H && px < W) ? c1_g(gy + (size_t)b * HW, y + (size_t)b * HW, (size_t)py * W + px) : 0.f;
                gsum += g[s][r][j];
            }
    float* out = partial + (size_t)blockIdx.x * n;
    c1_block_sum_to(gsum, red, 0);
    __syncthreads();
    if (threadIdx.x == 0) out[Ci * 9] = (red[0] + red[40]) + (red[80] + red[120]);
    for (int c0 = 0; c0 < Ci; c0 += C1_CC) {
        float acc[C1_CC][9];
#pragma unroll
        for (int cc = 0; cc < C1_CC; ++cc)
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[cc][k] = 0.f;
        for (int s = 0; s < C1_SUB; ++s) {
            const int y0 = (sy * C1_SUB + s) * C1_TY;
            if (y0 >= H) break;
            __syncthreads();
            c1_stage(Xs, xb, c0, Ci, H, W, y0, x0);
            __syncthreads();
#pragma unroll
            for (int cc = 0; cc < C1_CC; ++cc) {
                float win[4][6];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < 6; ++j) win[r][j] = Xs[cc * C1_PLANE + (ly + r) * C1_RS + lx + j];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                acc[cc][ky * 3 + kx] = fmaf(win[r + ky][j + kx], g[s][r][j], acc[cc][ky * 3 + kx]);
            }
        }
        __syncthreads();                                 // red[] of the previous step has been read
#pragma unroll
        for (int cc = 0; cc < C1_CC; ++cc)
#pragma unroll
            for (int k = 0; k < 9; ++k) c1_block_sum_to(acc[cc][k], red, cc * 9 + k);
        __syncthreads();
        if (threadIdx.x < C1_CC * 9) {
            const int cc = threadIdx.x / 9;
            if (c0 + cc < Ci)
                out[(c0 + cc) * 9 + threadIdx.x % 9] =
                    (red[threadIdx.x] + red[40 + threadIdx.x]) + (red[80 + threadIdx.x] + red[120 + threadIdx.x]);
        }
    }
}

// out[i] = sum_p partial[p][i] for i < n, fixed order: 4 waves take the rows p = wave, wave + 4, ..., then the waves in order.
// Deliberately not ecm_sum_partials (partial_sum.h): another order of additions (other bits), and the bias is split off here.
__global__ __launch_bounds__(256) void c1_reduce(const float* __restrict__ partial, float* __restrict__ gw,
                                                 float* __restrict__ gb, int n, int P) {
    __shared__ float sm[4][64];
    const int o = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + o;
    float s0 = 0.f, s1 = 0.f;
    if (i < n) {
        int p = wv;
        for (; p + 4 < P; p += 8) {
            s0 += partial[(size_t)p * n + i];
            s1 += partial[(size_t)(p + 4) * n + i];
        }
        for (; p < P; p += 4) s0 += partial[(size_t)p * n + i];
    }
    sm[wv][o] = s0 + s1;
    __syncthreads();
    if (wv == 0 && i < n) {
        const float t = (sm[0][o] + sm[1][o]) + (sm[2][o] + sm[3][o]);
        if (i == n - 1) gb[0] = t;
        else gw[i] = t;
    }
}

// ------------------------------------------------------------------------------------------- per-channel sum (bias grad)
// pass 1: partial[c][b * chunks + k] = sum of chunk k (C1_CHUNK floats) of plane (b, c); pass 2: out[c] = the B * chunks
// partials of channel c summed in order.
constexpr int C1_CHUNK = 16384;

__global__ __launch_bounds__(256) void chsum_partial(const float* __restrict__ x, float* __restrict__ partial, int C,
                                                     long long HW, int chunks) {
    __shared__ float red[4];
    const int k = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const float* p = x + ((size_t)b * C + c) * (size_t)HW;
    const long long lo = (long long)k * C1_CHUNK;
    const long long hi = lo + C1_CHUNK < HW ? lo + C1_CHUNK : HW;
    float s = 0.f;
    if ((HW & 3) == 0 && (reinterpret_cast<size_t>(x) & 15) == 0) {
        for (long long e = lo + threadIdx.x * 4; e < hi; e += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(p + e);
            s += (v.x + v.y) + (v.z + v.w);
        }
    } else {
        for (long long e = lo + threadIdx.x; e < hi; e += 256) s += p[e];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[((size_t)c * gridDim.z + b) * chunks + k] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void chsum_final(const float* __restrict__ partial, float* __restrict__ out, int m) {
    __shared__ float red[4];
    const float* p = partial + (size_t)blockIdx.x * m;
    float s = 0.f;
    for (int e = threadIdx.x; e < m; e += 256) s += p[e];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

inline bool c1_geom_ok(int B, int Ci, int H, int W) {
    if (B <= 0 || Ci <= 0 || H <= 0 || W <= 0) return false;
    const long long tiles = (long long)B * ((H + C1_TY - 1) / C1_TY) * ((W + C1_TX - 1) / C1_TX);
    return tiles <= 0x7fffffffLL && Ci <= 4096;
}

// The weight gradient's launch plan, read by its scratch query and its launcher: one workgroup, and one partial of
// n = Ci * 9 + 1 floats (the bias gradient last), per strip of C1_SUB tiles down the image.
struct C1WgPlan { int tiles_x, strips_y, n; long long P; };
inline C1WgPlan c1_wgrad_plan(int B, int Ci, int H, int W) {
    C1WgPlan p;
    p.tiles_x = (W + C1_TX - 1) / C1_TX;
    p.strips_y = (H + C1_TY * C1_SUB - 1) / (C1_TY * C1_SUB);
    p.P = (long long)B * p.strips_y * p.tiles_x;           // <= the tile count that c1_geom_ok bounds by 2^31
    p.n = Ci * 9 + 1;
    return p;
}

}  // namespace

extern "C" int ecm_conv2d_c1_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int H, int W,
                                 void* stream) {
    ECM_CHECK_ARG(x && w && bias && y && c1_geom_ok(B, Ci, H, W));
    const int tx = (W + C1_TX - 1) / C1_TX, ty = (H + C1_TY - 1) / C1_TY;
    hipLaunchKernelGGL(conv2d_c1_fwd, dim3((unsigned)((long long)B * tx * ty)), dim3(256), 0, ecm_stream(stream), x, w, bias, y,
                       Ci, H, W, tx, ty);
    return ECM_LAUNCH_RESULT();
}

extern "C" int ecm_conv2d_c1_dgrad(const float* gy, const float* y, const float* w, float* gx, int B, int Ci, int H, int W,
                                   void* stream) {
    ECM_CHECK_ARG(gy && y && w && gx && c1_geom_ok(B, Ci, H, W));
    const int tx = (W + C1_TX - 1) / C1_TX, ty = (H + C1_TY - 1) / C1_TY;
    hipLaunchKernelGGL(conv2d_c1_dgrad, dim3((unsigned)((long long)B * tx * ty)), dim3(256), 0, ecm_stream(stream), gy, y, w, gx,
                       Ci, H, W, tx, ty);
    return ECM_LAUNCH_RESULT();
}

extern "C" long long ecm_conv2d_c1_wgrad_scratch_bytes(int B, int Ci, int H, int W) {
    if (!c1_geom_ok(B, Ci, H, W)) return 0;
    const C1WgPlan p = c1_wgrad_plan(B, Ci, H, W);
    return p.P * p.n * (long long)sizeof(float);
}

extern "C" int ecm_conv2d_c1_wgrad(const float* x, const float* gy, const float* y, float* gw, float* gb, void* scratch,
                                   long long scratch_bytes, int B, int Ci, int H, int W, void* stream) {
    ECM_CHECK_ARG(x && gy && y && gw && gb && scratch && c1_geom_ok(B, Ci, H, W));
    const C1WgPlan p = c1_wgrad_plan(B, Ci, H, W);
    if (scratch_bytes < p.P * p.n * (long long)sizeof(float)) return ECM_ESCRATCH;
    hipStream_t st = ecm_stream(stream);
    float* partial = static_cast<float*>(scratch);
    hipLaunchKernelGGL(conv2d_c1_wgrad, dim3((unsigned)p.P), dim3(256), 0, st, x, gy, y, partial, Ci, H, W, p.tiles_x, p.strips_y);
    hipLaunchKernelGGL(c1_reduce, dim3((p.n + 63) / 64), dim3(256), 0, st, partial, gw, gb, p.n, (int)p.P);
    return ECM_LAUNCH_RESULT();
}

extern "C" long long ecm_channel_sum_scratch_bytes(int B, int C, long long HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return 0;
    return (long long)C * B * ((HW + C1_CHUNK - 1) / C1_CHUNK) * (long long)sizeof(float);
}

extern "C" int ecm_channel_sum(const float* x, float* out, void* scratch, long long scratch_bytes, int B, int C, long long HW,
                               void* stream) {
    ECM_CHECK_ARG(x && out && scratch && B > 0 && C > 0 && HW > 0);
    if (B > 65535 || C > 65535) return ECM_EUNSUP;
    const long long chunks = (HW + C1_CHUNK - 1) / C1_CHUNK;
    if (chunks * B > 0x7fffffffLL) return ECM_EUNSUP;
    if (scratch_bytes < ecm_channel_sum_scratch_bytes(B, C, HW)) return ECM_ESCRATCH;
    hipStream_t st = ecm_stream(stream);
    float* partial = static_cast<float*>(scratch);
    hipLaunchKernelGGL(chsum_partial, dim3((unsigned)chunks, C, B), dim3(256), 0, st, x, partial, C, HW, (int)chunks);
    hipLaunchKernelGGL(chsum_final, dim3(C), dim3(256), 0, st, partial, out, (int)(chunks * B));
    return ECM_LAUNCH_RESULT();
}
