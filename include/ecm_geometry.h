/*
 * ecm_geometry.h -- the geometry entries of libecm_hip.so: from a disparity map to 3-D points.
 *
 * A second header beside ecm_hip.h, with its own prefix (ecmg_): ecm_hip.h stays the ABI of the network and its post-filters.
 * The conventions are ecm_hip.h's: plain pointers and ints, every pointer a DEVICE pointer the caller owns, `stream` a
 * hipStream_t passed as void* (NULL = default stream), work enqueued asynchronously, 0 on success, a negative ECM_E* code of
 * ecm_hip.h on a bad argument (ecm_error_string names it) or the positive hipError_t of a failed launch.
 *
 * Definition (OpenCV's reprojectImageTo3D, evaluated in double).  For pixel (x, y) of image b with disparity d = disp[b,y,x]:
 *     [X Y Z W]^T = Q_b * [x y d 1]^T,    row r:  ((Q[r][0] * x + Q[r][1] * y) + Q[r][2] * d) + Q[r][3]
 *   every product and sum one IEEE fp64 operation, in that order, without fused multiply-adds; then
 *     point = (X / W, Y / W, Z / W), each a true fp64 division rounded once to fp32.
 *   Q: 16 doubles per image, row-major ([B,4,4], q_per_image != 0), or one matrix shared by the batch ([4,4], q_per_image == 0).
 * Usable pixel.  All of: d finite;  valid[b,y,x] != 0 (an unsigned char plane; NULL: all ones);  min_disp < d <= max_disp,
 *   compared in fp32 (max_disp may be +inf; min_disp must be finite);  W finite and non-zero.  Comparisons on the input bits.
 */
#ifndef ECM_GEOMETRY_H
#define ECM_GEOMETRY_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The dense point map, one launch.  xyz [B,3,H,W] fp32: the point of every usable pixel, +0.0 in all three planes elsewhere;
 * mask (unsigned char [B,H,W], may be NULL): 1 where usable, else 0.  No atomics: bit-reproducible.
 * ECM_EINVAL, before any device work: a null disp, Q or xyz, B, H or W < 1, min_disp not finite, max_disp NaN or below min_disp,
 * xyz or mask equal to disp or valid.  B * H * W >= 2^31 or B * ceil(H * W / ecmg_point_cloud_tile()) >= 2^24: ECM_EUNSUP,
 * before any launch. */
int ecmg_reproject_fwd(const float* disp, const unsigned char* valid, const double* Q, int q_per_image, float* xyz,
                       unsigned char* mask, int B, int H, int W, float min_disp, float max_disp, void* stream);

/* The packed point cloud: the usable pixels only, in row-major pixel order, image after image.
 *   attrs (fp32 [B,C,H,W], C in 0..4; NULL with C = 0): planes gathered beside the coordinates, bit for bit (e.g. the left image).
 *   points (fp32, room for B * H * W rows of 3 + C floats: the worst case): row offsets[b] + k is the k-th usable pixel of image
 *     b as (X/W, Y/W, Z/W, attrs[b,0..C-1,y,x]).  Rows at or beyond N = offsets[B] are not written.
 *   offsets (long long [B + 1]): offsets[0] = 0, offsets[b + 1] - offsets[b] the usable pixels of image b.
 *   xyz, mask (may each be NULL): the dense outputs of ecmg_reproject_fwd, bit for bit, written in the same pass.
 *   scratch: ecmg_point_cloud_scratch_bytes(B, H, W) bytes (one int per tile), written before it is read.
 * A tile is ecmg_point_cloud_tile() consecutive pixels of one image (the last tile of an image is partial).  Three launches on
 * `stream`: per-tile counts (wave ballots), an exclusive scan of the B * tiles counts by one workgroup, and the emit pass, which
 * recomputes the predicate and ranks each pixel by tile offset + the counts of the waves before it + its position in its
 * wave's ballot.  No workgroup waits for another and there are no atomics: the order is the pixel order whatever the scheduling,
 * bit-reproducible, and image b's rows do not depend on the other images.
 * Both queries need no GPU; the scratch query answers 0 for a shape the entry refuses.  ECM_EINVAL, before any device work: what
 * ecmg_reproject_fwd refuses, a null points, offsets or scratch, C outside 0..4, attrs null with C > 0, an output equal to an
 * input.  ECM_ESCRATCH: scratch_bytes too small.  ECM_EUNSUP as for ecmg_reproject_fwd. */
int       ecmg_point_cloud_tile(void);
long long ecmg_point_cloud_scratch_bytes(int B, int H, int W);
int ecmg_point_cloud_fwd(const float* disp, const unsigned char* valid, const double* Q, int q_per_image, const float* attrs, int C,
                         float* points, long long* offsets, float* xyz, unsigned char* mask, void* scratch, long long scratch_bytes,
                         int B, int H, int W, float min_disp, float max_disp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_GEOMETRY_H */
