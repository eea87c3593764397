/*
 * ecm_motion.h -- the motion entries of libecm_hip.so: the normal equations of one Gauss-Newton step of the dense alignment of
 * two disparity maps by a rigid camera motion.
 *
 * A fifth header beside ecm_hip.h, ecm_geometry.h, ecm_rectify.h and ecm_temporal.h, with its own prefix (ecmm_).  The
 * conventions are ecm_hip.h's: plain pointers and ints, every pointer a DEVICE pointer the caller owns, `stream` a hipStream_t
 * passed as void* (NULL = default stream), work enqueued asynchronously, 0 on success, a negative ECM_E* code of ecm_hip.h on a
 * bad argument (ecm_error_string names it) or the positive hipError_t of a failed launch.
 *
 * Operands.  disp0 [B,H,W] fp32, the source map (the previous frame, or a carried state); disp1 [B,H,W] fp32, the target (this
 *   frame); valid0, valid1 unsigned char planes (NULL: all ones); weight0 [B,H,W] fp32, the inverse variance of the residual
 *   (NULL: 1).  Three fp64 4x4 row-major matrices: Q, the source view's disparity-to-depth matrix of ecm_geometry.h; Qinv_out,
 *   the INVERSE of the target view's; T, the current estimate of the motion that takes points of the source frame to the target
 *   frame, one for the batch ([4,4], t_per_image == 0) or one per image ([B,4,4], t_per_image != 0).  T's bottom row is not read.
 * Every operation below is one IEEE fp64 operation in the stated order, without fused multiply-adds, unless it says fp32.
 * Lattice.  Source pixels (x, y) with x % step == 0 and y % step == 0 are visited, row-major; the others take no part.
 * Usable source pixel.  ecm_geometry.h's rule on d = disp0[b,y,x]: d finite; valid0 != 0; min_disp < d <= max_disp, compared in
 *   fp32 (max_disp may be +inf);  P = Q [x y d 1]^T, row r: ((Q[r][0] * x + Q[r][1] * y) + Q[r][2] * d) + Q[r][3], and P[3] finite and
 *   non-zero.  And its weight w = weight0[b,y,x] (1 for NULL) is finite and > 0.
 * Projection.  X = P[0:3] / P[3] (three divisions);  Y[i] = ((T[i][0] * X[0] + T[i][1] * X[1]) + T[i][2] * X[2]) + T[i][3];
 *   h[r] = ((A[r][0] * Y[0] + A[r][1] * Y[1]) + A[r][2] * Y[2]) + A[r][3] with A = Qinv_out;  u = h[0] / h[3], v = h[1] / h[3],
 *   dn = h[2] / h[3].
 * Candidate.  A usable source pixel for which u, v and dn are finite, dn > 0, 0 <= u <= W-1 and 0 <= v <= H-1.
 * Target sample.  x0 = min(floor(u), W-2), y0 = min(floor(v), H-2), fx = u - x0, fy = v - y0 (so u == W-1 samples the last column
 *   with fx == 1).  The taps d00 = disp1[b,y0,x0], d01 = [y0,x0+1], d10 = [y0+1,x0], d11 = [y0+1,x0+1] must each be finite, have
 *   valid1 != 0 and lie in min_disp < d <= max_disp (fp32), and the largest minus the smallest must not exceed tap_range (a depth
 *   edge is not interpolated across); otherwise the pixel is dropped.  With the taps as doubles:
 *     top = d00 + fx * (d01 - d00);  bot = d10 + fx * (d11 - d10);  s = top + fy * (bot - top);
 *     gx = (1 - fy) * (d01 - d00) + fy * (d11 - d10);      gy = (1 - fx) * (d10 - d00) + fx * (d11 - d01).
 * Residual.  r = s - dn; the pixel is dropped unless |r| <= max_residual.  What is left is a USED pixel.
 * Jacobian of r with respect to a left-multiplied twist xi = (nu, omega), T <- exp(xi^) T, at xi = 0:  dY = [I | -[Y]x], so for
 *   each row q of A:  dh[q] = (A[q][0], A[q][1], A[q][2], A[q][2] * Y[1] - A[q][1] * Y[2], A[q][0] * Y[2] - A[q][2] * Y[0],
 *   A[q][1] * Y[0] - A[q][0] * Y[1]);   du[j] = (dh[0][j] - u * dh[3][j]) / h[3], dv[j] = (dh[1][j] - v * dh[3][j]) / h[3],
 *   dd[j] = (dh[2][j] - dn * dh[3][j]) / h[3];   J[j] = (gx * du[j] + gy * dv[j]) - dd[j],  j = 0..5.
 * Robust weight (Cauchy; a division only):  k = 1 / (1 + ((w * r) * r) / (cauchy * cauchy)), cauchy widened to fp64 first;  a = k * w.
 * Sums per image, ecmm_align_sums() == 32 doubles, over the used pixels:
 *   [0..20]  the upper triangle of sum (a * J[j]) * J[i], row-major (j <= i: 00 01 .. 05 11 12 .. 55);
 *   [21..26] sum (a * J[j]) * r;     [27] sum (a * r) * r;     [28] sum a;
 *   [29] the number of used pixels;  [30] the number of candidates;  [31] 0.
 *   The order of the additions is fixed (see below) but is not part of this definition: a restatement that adds in another order
 *   differs by at most n * 2^-52 * sum |term| per entry, n the number of terms.
 * residual [B,H,W] fp32 (may be NULL): (float) r at the used source pixels and a NaN (all bits set) everywhere else.
 */
#ifndef ECM_MOTION_H
#define ECM_MOTION_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The normal equations of one step.  scratch: ecmm_align_scratch_bytes(B, H, W, step) bytes, 8-byte aligned: one partial of 32
 * doubles per tile.  On `stream`: where residual is given, a hipMemsetAsync of it; an accumulating pass, in which a workgroup of
 * 256 takes one tile of 2048 consecutive lattice pixels of one image (ecmt_disparity_warp_fwd's tiling: item k of thread t is
 * lattice pixel k * 256 + t of the tile), every thread adds its eight pixels in order into registers, a wave adds its 64 lanes
 * in a fixed butterfly, the four waves are added in wave order through LDS, and the workgroup stores its partial; a finishing
 * pass, one workgroup per image, which adds that image's partials in a fixed order into sums[b].  No atomics, and no workgroup
 * waits for another: the result is bit-reproducible, and image b's sums do not depend on the other images of the batch.
 * Both queries need no GPU; the scratch query answers 0 for a shape the entry refuses.  ECM_EINVAL, before any device work: a
 * null disp0, disp1, Q, Qinv_out, T, sums or scratch, B < 1, H or W < 2, step < 1, min_disp not finite, max_disp NaN or below
 * min_disp, tap_range, max_residual or cauchy not finite or not > 0, sums, residual or scratch equal to one of the inputs or to
 * one another.  ECM_EUNSUP, before any launch: H * W >= 2^31, or B * ceil(ceil(H / step) * ceil(W / step) / 2048) >= 2^24.
 * ECM_ESCRATCH: scratch_bytes too small. */
int       ecmm_align_sums(void);
long long ecmm_align_scratch_bytes(int B, int H, int W, int step);
int ecmm_align_normal_fwd(const float* disp0, const unsigned char* valid0, const float* weight0, const float* disp1,
                          const unsigned char* valid1, const double* Q, const double* Qinv_out, const double* T, int t_per_image,
                          double* sums, float* residual, void* scratch, long long scratch_bytes, int B, int H, int W, int step,
                          float min_disp, float max_disp, float tap_range, float max_residual, float cauchy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_MOTION_H */
