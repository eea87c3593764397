/*
 * ecm_color.h -- the colour entries of libecm_hip.so: up to four attribute planes (colour, or anything else that is averaged)
 * carried in a TSDF volume (ecm_volume.h): integrated with the disparity maps, raycast back with them, and sampled at points such
 * as the vertices of the volume's mesh (ecm_mesh.h).  DESIGN.md section 36.
 *
 * An eighth header beside ecm_hip.h, ecm_geometry.h, ecm_rectify.h, ecm_temporal.h, ecm_motion.h, ecm_volume.h and ecm_mesh.h,
 * with its own prefix (ecmc_).  The conventions are ecm_hip.h's: plain pointers and ints, every pointer a DEVICE pointer the caller
 * owns, `stream` a hipStream_t passed as void* (NULL = default stream), work enqueued asynchronously, 0 on success, a negative
 * ECM_E* code of ecm_hip.h on a bad argument (ecm_error_string names it) or the positive hipError_t of a failed launch.
 *
 * Every operation below is one IEEE fp64 operation in the stated order, without fused multiply-adds, unless it says fp32; an fp32
 * operand of an fp64 operation is widened first, and (float) rounds once to nearest.  row(M, r, a, b, c) is ecm_volume.h's:
 * ((M[r][0] * a + M[r][1] * b) + M[r][2] * c) + M[r][3].
 *
 * Attribute volume.  Beside tsdf and wsum [nz,ny,nx] of ecm_volume.h: attr [A,nz,ny,nx] fp32, A planes of nz * ny * nx values one
 *   after another, 1 <= A <= ecmc_max_attributes(), and asum [nz,ny,nx] fp32, the weight the attributes were averaged over.  An
 *   empty volume is all zeros.  Grid points are indexed as in ecm_volume.h: (i, j, k) -- i along x -- at (k * ny + j) * nx + i.
 *
 * Integration.  For every voxel (i, j, k), the views v = 0 .. V-1 in that order, each acting on what the one before it left.  The
 *   geometry step is ecm_volume.h's Integration, word for word: the same skips, the same s = z_meas - z_vox, the same update of
 *   tsdf and wsum; they come out bit-identical to ecmv_integrate_fwd on the same operands.  The attribute step runs where the
 *   view is not skipped and, in addition, s <= trunc compared in fp64 (the voxel is then within trunc of the measured surface, on
 *   either side), and all A values c[a] = attributes[v,a,py,px] are finite (attributes is [V,A,H,W] fp32; (px, py) is the pixel
 *   the geometry step read, w its weight).  Then in fp32, with Y = attr[a,k,j,i] and Na = asum[k,j,i]:
 *     An = Na + w;   attr[a,k,j,i] = (Y * Na + c[a] * w) / An for each a;   asum[k,j,i] = min(An, max_weight).
 *   Otherwise the voxel's attr and asum keep their bits.
 *
 * Sampling rule (the raycast and the point sampling share it).  At a grid position g inside the box, per axis with dim = nx, ny,
 *   nz:  c = min(max(floor(g), 0), dim-2);  q = g - c.  The eight weights are b[dz][dy][dx] = (fz * fy) * fx, where a factor is
 *   1 - q on its axis for the corner offset 0 and q for the offset 1.  With num[a] = 0 and den = 0, over the corners in the
 *   order dz, dy, dx (dx fastest), using only the corners with asum > 0 (fp32; a NaN fails):
 *     num[a] = num[a] + b * attr[a] at the corner, for each a;   den = den + b.
 *   The value is (float)(num[a] / den), or +0.0 for every a where den == 0.  It is a normalised blend: a corner that was never
 *   coloured does not darken its neighbours.
 *
 * Raycast.  ecm_volume.h's Raycast, unchanged: out and hit_weight are bit-identical to ecmv_raycast_fwd on the same operands.
 *   colors[b,a,y,x] ([B,A,H,W] fp32) holds the sampling rule at the hit p*; a hole is +0.0 in every plane.
 *
 * Point sampling.  For point n = (x, y, z) of points [N,3] fp32:  g[r] = row(Minv, r, x, y, z), r = 0..2.  Minv is an fp64 4x4
 *   row-major output-to-grid matrix whose bottom row is (0, 0, 0, 1) and is not read.  The point is OUTSIDE iff some g[r] is not
 *   finite, or g[r] < -0.5 or g[r] > dim - 0.5 on some axis (half a voxel beyond the outermost grid points).  Otherwise g is
 *   clamped into [0, dim-1] per axis, min(max(g, 0), dim-1), and out[n,a] ([N,A] fp32) is the sampling rule there.  An outside
 *   point gets +0.0 in every out[n,a].
 */
#ifndef ECM_COLOR_H
#define ECM_COLOR_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest A the entries below take: 4, as ecmt_disparity_warp_max_attributes().  No GPU needed. */
int ecmc_max_attributes(void);

/* Integrate V views and their attributes into the volume, in place, in one launch of ecmv_integrate_fwd's geometry: one thread
 * per voxel (four voxels along x where nx % 4 == 0 and tsdf, wsum, attr and asum are all 16-byte aligned; else one), the view loop
 * inside the thread, so that every one of the 2 + A + 1 planes is read once and written once.  No atomics, no workgroup waits
 * for another, no scratch: bit-reproducible.
 * ECM_EINVAL, before any device work: a null tsdf, wsum, attr, asum, disp, attributes, Q, G or C; nx, ny, nz, V, H or W < 1;
 * trunc or max_weight not finite or not > 0; min_disp not finite; max_disp NaN or below min_disp; tsdf, wsum, attr or asum equal
 * to one another or to one of the inputs.  ECM_EUNSUP, before any launch: A outside 1..ecmc_max_attributes(); nx * ny * nz >= 2^31,
 * H * W >= 2^31, or 2^24 bricks or more (a brick is 16 x 4 x 4 threads). */
int ecmc_integrate_fwd(float* tsdf, float* wsum, float* attr, float* asum, const float* disp, const unsigned char* valid,
                       const float* weight, const float* attributes, const double* Q, const double* G, const double* C, int m_per_view,
                       int nx, int ny, int nz, int A, int V, int H, int W, float trunc, float max_weight, float min_disp, float max_disp,
                       void* stream);

/* Raycast the volume and its attributes from B views in one launch: out [B,H,W] fp32, colors [B,A,H,W] fp32 and, where given,
 * hit_weight [B,H,W] fp32.  ecmv_raycast_fwd's launch: one thread per pixel, a workgroup of 256 on a tile of 16 x 16 pixels, each
 * wave on 8 x 8 of them.  No atomics, no scratch: bit-reproducible, and view b does not depend on the others.
 * ECM_EINVAL, before any device work: a null tsdf, wsum, attr, asum, R, Rinv, out or colors; nx, ny or nz < 2; B, H or W < 1;
 * max_steps < 1; step not finite or not > 0; near_disp or far_disp not finite, or not near_disp > far_disp > 0; out, hit_weight
 * or colors equal to one another or to one of the inputs.  ECM_EUNSUP, before any launch: A outside 1..ecmc_max_attributes();
 * nx * ny * nz >= 2^31, H * W >= 2^31, B * ceil(H / 16) * ceil(W / 16) >= 2^24, or max_steps > ecmv_raycast_max_steps(). */
int ecmc_raycast_fwd(const float* tsdf, const float* wsum, const float* attr, const float* asum, const double* R, const double* Rinv,
                     int m_per_view, float* out, float* hit_weight, float* colors, int nx, int ny, int nz, int A, int B, int H, int W,
                     float near_disp, float far_disp, float step, int max_steps, void* stream);

/* Sample the attributes at N points in one launch: out [N,A] fp32.  One thread per point, workgroups of 256.  No atomics, no
 * scratch: bit-reproducible.
 * ECM_EINVAL, before any device work: a null attr, asum, Minv, points or out; N < 1; nx, ny or nz < 2; out equal to one of the
 * inputs.  ECM_EUNSUP, before any launch: A outside 1..ecmc_max_attributes(); N >= 2^31; nx * ny * nz >= 2^31. */
int ecmc_sample_fwd(const float* attr, const float* asum, const double* Minv, const float* points, float* out, long long N, int nx,
                    int ny, int nz, int A, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_COLOR_H */
