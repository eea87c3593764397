// Dense disparity alignment (include/ecm_motion.h has the definitions): the normal equations of one
// Gauss-Newton step for the rigid motion that maps one disparity map onto the next -- per lattice pixel an fp64 projection
// through Q, T and Q_out^-1, a four-tap gather of the target map, a 1x6 Jacobian and 31 sums.
// A workgroup owns one linear pixel tile (disp_geom.h) of LATTICE pixels: the matrices are uniform per workgroup.
//   accumulate  every thread adds its items, in order, into 29 fp64 accumulators and two counters in registers; a wave adds its
//               64 lanes in a fixed xor butterfly (a + b is commutative: every lane holds the same bits), the four waves are
//               added in wave order through LDS, and the workgroup stores one partial of 32 doubles;
//   finish      one workgroup per image: partial_sum.h's pattern restated for doubles -- 8 lane groups each add every 8th
//               partial into four accumulators, and the 8 group sums are added in order.
// No atomics, no workgroup waits for another, no dependence on the batch: bit-reproducible.  The whole file is compiled with
// contraction off: every product and sum is one fp64 operation, as the header states them.
#include "disp_geom.h"
#include "../../include/ecm_motion.h"

#pragma clang fp contract(off)

namespace {

using namespace ecm_pix;
constexpr int SUMS = 32;                      // doubles per partial and per image
constexpr int ACCS = 29;                      // 21 of J^T J, 6 of J^T r, r^2 and the weight

struct Gates {
    DispRange range;
    double tap_range, max_residual, c2;       // c2 = cauchy^2
};

// ---- accumulate ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void align_accumulate(const float* __restrict__ disp0, const unsigned char* __restrict__ valid0,
                                                            const float* __restrict__ weight0, const float* __restrict__ disp1,
                                                            const unsigned char* __restrict__ valid1, const double* __restrict__ Q,
                                                            const double* __restrict__ A, const double* __restrict__ Tm, int t_stride,
                                                            double* __restrict__ partial, float* __restrict__ residual, int W, int H,
                                                            int Ws, int L, int tiles, int step, Gates g) {
    const PixTile t = ecm_pix_tile(tiles);
    const double* __restrict__ T = Tm + (size_t)t.b * t_stride;
    const size_t img = (size_t)t.b * H * W;
    const double inf = __builtin_inf(), last_x = (double)(W - 1), last_y = (double)(H - 1);

    double acc[ACCS];
#pragma unroll
    for (int i = 0; i < ACCS; ++i) acc[i] = 0.0;
    int used = 0, cand = 0;

#pragma unroll 1
    for (int k = 0; k < ITEMS; ++k) {
        const unsigned l = t.first + k * THREADS + threadIdx.x;
        if (l >= (unsigned)L) continue;
        int lx, ly;
        ecm_pix_xy(l, Ws, lx, ly);
        const int x = lx * step, y = ly * step;                            // x <= W-1, y <= H-1: Ws = ceil(W / step), L = Hs * Ws
        const size_t pix = img + (size_t)y * W + x;
        const float d = disp0[pix];
        if (!ecm_disp_usable(d, !valid0 || valid0[pix] != 0, g.range)) continue;
        const double w = weight0 ? (double)weight0[pix] : 1.0;
        if (!(w > 0.0 && w < inf)) continue;
        const double fxs = (double)x, fys = (double)y, fd = (double)d;
        const double P3 = ecm_row4(Q + 12, fxs, fys, fd);
        if (!ecm_nonzero_finite(P3)) continue;
        const double X0 = ecm_row4(Q, fxs, fys, fd) / P3, X1 = ecm_row4(Q + 4, fxs, fys, fd) / P3, X2 = ecm_row4(Q + 8, fxs, fys, fd) / P3;
        const double Y0 = ((T[0] * X0 + T[1] * X1) + T[2] * X2) + T[3];
        const double Y1 = ((T[4] * X0 + T[5] * X1) + T[6] * X2) + T[7];
        const double Y2 = ((T[8] * X0 + T[9] * X1) + T[10] * X2) + T[11];
        const double h3 = ecm_row4(A + 12, Y0, Y1, Y2);
        const double u = ecm_row4(A, Y0, Y1, Y2) / h3, v = ecm_row4(A + 4, Y0, Y1, Y2) / h3, dn = ecm_row4(A + 8, Y0, Y1, Y2) / h3;
        // every comparison fails on a NaN; u and v inside the image are finite
        if (!(fabs(dn) < inf && dn > 0.0 && u >= 0.0 && u <= last_x && v >= 0.0 && v <= last_y)) continue;
        ++cand;
        const int x0 = min((int)floor(u), W - 2), y0 = min((int)floor(v), H - 2);      // 0 <= x0 <= W-2, 0 <= y0 <= H-2: W, H >= 2
        const double fx = u - (double)x0, fy = v - (double)y0;
        const size_t at = img + (size_t)y0 * W + x0;
        const float t00 = disp1[at], t01 = disp1[at + 1], t10 = disp1[at + W], t11 = disp1[at + W + 1];
        const bool v00 = !valid1 || valid1[at] != 0, v01 = !valid1 || valid1[at + 1] != 0;
        const bool v10 = !valid1 || valid1[at + W] != 0, v11 = !valid1 || valid1[at + W + 1] != 0;
        if (!(ecm_disp_usable(t00, v00, g.range) && ecm_disp_usable(t01, v01, g.range) && ecm_disp_usable(t10, v10, g.range) &&
              ecm_disp_usable(t11, v11, g.range)))
            continue;
        const float hi = fmaxf(fmaxf(t00, t01), fmaxf(t10, t11)), lo = fminf(fminf(t00, t01), fminf(t10, t11));
        if ((double)hi - (double)lo > g.tap_range) continue;
        const double d00 = t00, d01 = t01, d10 = t10, d11 = t11;
        const double top = d00 + fx * (d01 - d00), bot = d10 + fx * (d11 - d10);
        const double s = top + fy * (bot - top);
        const double gx = (1.0 - fy) * (d01 - d00) + fy * (d11 - d10);
        const double gy = (1.0 - fx) * (d10 - d00) + fx * (d11 - d01);
        const double r = s - dn;
        if (!(fabs(r) <= g.max_residual)) continue;
        ++used;
        if (residual) residual[pix] = (float)r;

        double J[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double dh[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double a0 = A[4 * q], a1 = A[4 * q + 1], a2 = A[4 * q + 2];
                dh[q] = j == 0 ? a0 : j == 1 ? a1 : j == 2 ? a2 : j == 3 ? a2 * Y1 - a1 * Y2 : j == 4 ? a0 * Y2 - a2 * Y0 : a1 * Y0 - a0 * Y1;
            }
            const double du = (dh[0] - u * dh[3]) / h3, dv = (dh[1] - v * dh[3]) / h3, dd = (dh[2] - dn * dh[3]) / h3;
            J[j] = (gx * du + gy * dv) - dd;
        }
        const double kc = 1.0 / (1.0 + ((w * r) * r) / g.c2);
        const double a = kc * w;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double aj = a * J[j];
#pragma unroll
            for (int i = j; i < 6; ++i) acc[j * 6 - j * (j - 1) / 2 + (i - j)] += aj * J[i];      // row j of the upper triangle starts at 6j - j(j-1)/2
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[21 + j] += (a * J[j]) * r;
        acc[27] += (a * r) * r;
        acc[28] += a;
    }

    __shared__ double sm[NWAVE][SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < ACCS; ++i) {
        const double s = wave_sum(acc[i]);
        if (lane == 0) sm[wave][i] = s;
    }
    const double n_used = wave_sum((double)used), n_cand = wave_sum((double)cand);   // integers below 2^53: exact
    if (lane == 0) {
        sm[wave][29] = n_used;
        sm[wave][30] = n_cand;
        sm[wave][31] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < SUMS) {
        const int i = threadIdx.x;
        partial[(size_t)blockIdx.x * SUMS + i] = ((sm[0][i] + sm[1][i]) + sm[2][i]) + sm[3][i];
    }
}

// ---- finish ------------------------------------------------------------------------------------------------------------------
// sums[b][o] = sum_p partial[b][p][o]: partial_sum.h's order of additions, in doubles
__global__ __launch_bounds__(THREADS) void align_finish(const double* __restrict__ partial, double* __restrict__ sums, int tiles) {
    const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const double* __restrict__ src = partial + (size_t)blockIdx.x * tiles * SUMS + o;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int p = grp;
    for (; p < tiles - 24; p += 32) {                                      // four strides of 8 at a time, then the tail
        s0 += src[(size_t)p * SUMS];
        s1 += src[(size_t)(p + 8) * SUMS];
        s2 += src[(size_t)(p + 16) * SUMS];
        s3 += src[(size_t)(p + 24) * SUMS];
    }
    for (; p < tiles; p += 8) s0 += src[(size_t)p * SUMS];
    __shared__ double groups[8][SUMS];
    groups[grp][o] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (grp == 0) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += groups[q][o];
        sums[(size_t)blockIdx.x * SUMS + o] = t;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// tiles per image, or 0 where the shape is refused (code: why)
int tiles_per_image(int B, int H, int W, int step, int& code) {
    code = ECM_EINVAL;
    if (B < 1 || H < 2 || W < 2 || step < 1) return 0;
    code = ECM_EUNSUP;
    const long long hw = (long long)H * W;
    if (hw > INT_MAX) return 0;               // the image, not the batch: ecm_motion.h states H * W, and img is a size_t
    const long long hs = ((long long)H + step - 1) / step, ws = ((long long)W + step - 1) / step;
    return ecm_pix_tiles(hs * ws, B, code);
}

}  // namespace

extern "C" int ecmm_align_sums(void) { return SUMS; }

extern "C" long long ecmm_align_scratch_bytes(int B, int H, int W, int step) {
    int code;
    const int T = tiles_per_image(B, H, W, step, code);
    return (long long)B * T * SUMS * (long long)sizeof(double);
}

extern "C" int ecmm_align_normal_fwd(const float* disp0, const unsigned char* valid0, const float* weight0, const float* disp1,
                                     const unsigned char* valid1, const double* Q, const double* Qinv_out, const double* T,
                                     int t_per_image, double* sums, float* residual, void* scratch, long long scratch_bytes, int B,
                                     int H, int W, int step, float min_disp, float max_disp, float tap_range, float max_residual,
                                     float cauchy, void* stream) {
    ECM_CHECK_ARG(disp0 && disp1 && Q && Qinv_out && T && sums && scratch);
    ECM_CHECK_ARG(ecm_disp_range_ok(min_disp, max_disp));
    ECM_CHECK_ARG(ecm_positive(tap_range) && ecm_positive(max_residual) && ecm_positive(cauchy));
    ECM_CHECK_ARG(ecm_no_alias({sums, residual, scratch}, {disp0, valid0, weight0, disp1, valid1, Q, Qinv_out, T}));
    ECM_CHECK_ARG((const void*)sums != (const void*)residual && (const void*)sums != scratch && (const void*)residual != scratch);
    int code;
    const int tiles = tiles_per_image(B, H, W, step, code);
    if (!tiles) return code;
    if (scratch_bytes < ecmm_align_scratch_bytes(B, H, W, step)) return ECM_ESCRATCH;
    const int Hs = (int)(((long long)H + step - 1) / step), Ws = (int)(((long long)W + step - 1) / step);
    const Gates g = {{min_disp, max_disp}, (double)tap_range, (double)max_residual, (double)cauchy * (double)cauchy};
    double* partial = static_cast<double*>(scratch);
    hipStream_t s = ecm_stream(stream);
    if (residual) {
        const hipError_t filled = hipMemsetAsync(residual, 0xff, (size_t)B * H * W * sizeof(float), s);
        if (filled != hipSuccess) return (int)filled;
    }
    hipLaunchKernelGGL(align_accumulate, dim3(B * tiles), dim3(THREADS), 0, s, disp0, valid0, weight0, disp1, valid1, Q, Qinv_out, T,
                       ecm_mat_stride(t_per_image), partial, residual, W, H, Ws, Hs * Ws, tiles, step, g);
    hipLaunchKernelGGL(align_finish, dim3(B), dim3(THREADS), 0, s, (const double*)partial, sums, tiles);
    return ECM_LAUNCH_RESULT();
}
