/*
 * ecm_volume.h -- the volume entries of libecm_hip.so: a truncated signed distance (TSDF) volume that disparity maps are
 * integrated into, view after view, and raycast back out of as a disparity map from any pose.
 *
 * A sixth header beside ecm_hip.h, ecm_geometry.h, ecm_rectify.h, ecm_temporal.h and ecm_motion.h, with its own prefix (ecmv_).
 * The conventions are ecm_hip.h's: plain pointers and ints, every pointer a DEVICE pointer the caller owns, `stream` a hipStream_t
 * passed as void* (NULL = default stream), work enqueued asynchronously, 0 on success, a negative ECM_E* code of ecm_hip.h on a
 * bad argument (ecm_error_string names it) or the positive hipError_t of a failed launch.
 *
 * Volume.  Two fp32 planes of nz * ny * nx values, x fastest: tsdf [nz,ny,nx], the truncated signed distance in units of trunc
 *   (in [-1, 1], positive in front of a surface), and wsum [nz,ny,nx], the weight it was averaged over.  An empty volume is
 *   tsdf = 1 and wsum = 0.  Grid point (i, j, k) -- i along x -- is the world point origin + voxel * (i, j, k).
 * Matrices.  fp64 4x4, row-major, built on the host from S = [[voxel * I, origin], [0, 1]] (grid to world), the pose T of a view
 *   (world to camera) and the view's disparity-to-depth matrix Q of ecm_geometry.h:  C = T S (grid to camera),  G = inv(Q) C (grid
 *   to (u, v, d)),  R = inv(S) inv(T) Q ((x, y, d) to grid),  Rinv = inv(R).  One set for all views ([4,4], m_per_view == 0) or one
 *   per view ([V,4,4], m_per_view != 0).  row(M, r, a, b, c) = ((M[r][0] * a + M[r][1] * b) + M[r][2] * c) + M[r][3].
 * Every operation below is one IEEE fp64 operation in the stated order, without fused multiply-adds, unless it says fp32; an fp32
 * operand of an fp64 operation is widened first, and (float) rounds once to nearest.
 *
 * Integration.  For every voxel (i, j, k), the views v = 0 .. V-1 in that order, each acting on what the one before it left:
 *   h[r] = row(G_v, r, i, j, k), r = 0..3;  u = h[0] / h[3], v = h[1] / h[3], dv = h[2] / h[3];  the view is skipped unless all
 *   three are finite and dv > 0.  px = floor(u + 0.5), py = floor(v + 0.5); skipped unless 0 <= px <= W-1 and 0 <= py <= H-1.
 *   d = disp[v,py,px] must be usable by ecm_geometry.h's rule: d finite, valid[v,py,px] != 0 (NULL: all ones), min_disp < d <=
 *   max_disp compared in fp32, and P[3] = row(Q, 3, px, py, d) finite and non-zero; and w = weight[v,py,px] (NULL: 1) must be finite
 *   and > 0; otherwise the view is skipped.  z_meas = row(Q, 2, px, py, d) / P[3];  z_vox = row(C_v, 2, i, j, k); skipped unless both
 *   are finite and > 0.  s = z_meas - z_vox, the distance ALONG THE OPTICAL AXIS; skipped if s < -trunc (the voxel lies more than
 *   trunc behind the surface).  t = (float) min(1, s / trunc).  Then in fp32, with X = tsdf[k,j,i] and N = wsum[k,j,i]:
 *     Wn = N + w;   tsdf[k,j,i] = (X * N + t * w) / Wn;   wsum[k,j,i] = min(Wn, max_weight).
 *   A voxel that every view skips keeps its two values bit for bit.
 *
 * Raycast.  For every pixel (x, y) of view b:  gn[a] = row(R_b, a, x, y, near_disp) / row(R_b, 3, x, y, near_disp), a = 0..2, and gf
 *   likewise at far_disp;  dir = gf - gn;  len = sqrt((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]);  n = ceil(len / step).
 *   The pixel is a hole unless gn, gf and n are finite and 1 <= n <= max_steps.  Sample m = 0 .. n is p_m = gn + dir * (m / n), per
 *   axis.  A sample is VALID iff c = floor(p_m) has 0 <= c <= dim-2 on each axis (dim = nx, ny, nz) and the eight wsum at
 *   c + {0,1}^3 are > 0.  Its value f_m is the blend of the eight tsdf, t[dz][dy][dx] widened, with q = p_m - c:
 *     a[dz][dy] = t[dz][dy][0] + q[0] * (t[dz][dy][1] - t[dz][dy][0]);   e[dz] = a[dz][0] + q[1] * (a[dz][1] - a[dz][0]);
 *     f = e[0] + q[2] * (e[1] - e[0]).
 *   Going up from m = 1, the first pair (m-1, m) of valid samples with f0 = f_(m-1) > 0 and f1 = f_m <= 0 is the HIT:
 *     a = f0 / (f0 - f1);   p* = p_(m-1) + (p_m - p_(m-1)) * a;   hh[r] = row(Rinv_b, r, p*[0], p*[1], p*[2]);
 *     out[b,y,x] = (float)(hh[2] / hh[3]).
 *   A pair of valid samples with f0 < 0 and f1 > 0 (a back face) met before a hit ends the ray as a hole; an invalid sample is
 *   part of no pair.  A hole is +0.0 in out and in hit_weight.  hit_weight[b,y,x] (may be NULL) is, at a hit, (float) of the same
 *   blend of the eight wsum about p*, in the cell min(max(floor(p*), 0), dim-2).
 *   A sample outside the box 0 <= p < dim-1 is invalid by the rule above, so a kernel may leave out samples that lie outside it;
 *   it visits every other sample.
 */
#ifndef ECM_VOLUME_H
#define ECM_VOLUME_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Integrate V views into the volume, in place, in one launch: one thread per voxel (four voxels along x where nx % 4 == 0 and
 * both planes are 16-byte aligned), the view loop inside the thread, so that a voxel is read once and written once.  A workgroup
 * of 256 owns a brick of 16 x 4 x 4 threads.  No atomics, no workgroup waits for another, no scratch: bit-reproducible.
 * ECM_EINVAL, before any device work: a null tsdf, wsum, disp, Q, G or C; nx, ny, nz, V, H or W < 1; trunc or max_weight not
 * finite or not > 0; min_disp not finite; max_disp NaN or below min_disp; tsdf or wsum equal to one another or to one of the
 * inputs.  ECM_EUNSUP, before any launch: nx * ny * nz >= 2^31, H * W >= 2^31, or 2^24 bricks or more. */
int ecmv_integrate_fwd(float* tsdf, float* wsum, const float* disp, const unsigned char* valid, const float* weight, const double* Q,
                       const double* G, const double* C, int m_per_view, int nx, int ny, int nz, int V, int H, int W, float trunc,
                       float max_weight, float min_disp, float max_disp, void* stream);

/* The largest max_steps ecmv_raycast_fwd takes: 65536.  No GPU needed. */
int ecmv_raycast_max_steps(void);

/* Raycast the volume from B views in one launch: out [B,H,W] fp32 and, where given, hit_weight [B,H,W] fp32.  One thread per
 * pixel, a workgroup of 256 on a tile of 16 x 16 pixels, each wave on 8 x 8 of them; the samples before the ray enters the
 * volume's box and after it leaves are left out.  No atomics, no scratch: bit-reproducible, and view b does not depend on the others.
 * ECM_EINVAL, before any device work: a null tsdf, wsum, R, Rinv or out; nx, ny or nz < 2; B, H or W < 1; max_steps < 1; step not
 * finite or not > 0; near_disp or far_disp not finite, or not near_disp > far_disp > 0; out or hit_weight equal to one another
 * or to one of the inputs.  ECM_EUNSUP, before any launch: nx * ny * nz >= 2^31, H * W >= 2^31,
 * B * ceil(H / 16) * ceil(W / 16) >= 2^24, or max_steps > ecmv_raycast_max_steps(). */
int ecmv_raycast_fwd(const float* tsdf, const float* wsum, const double* R, const double* Rinv, int m_per_view, float* out,
                     float* hit_weight, int nx, int ny, int nz, int B, int H, int W, float near_disp, float far_disp, float step,
                     int max_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_VOLUME_H */
