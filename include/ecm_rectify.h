/*
 * ecm_rectify.h -- the rectification entries of libecm_hip.so: from a raw, distorted camera pair to the network's inputs
 * (DESIGN.md section 24).
 *
 * A third header beside ecm_hip.h and ecm_geometry.h, with its own prefix (ecmr_).  The conventions are ecm_hip.h's: plain
 * pointers and ints, every pointer a DEVICE pointer the caller owns unless it is called a HOST array, `stream` a hipStream_t
 * passed as void* (NULL = default stream), work enqueued asynchronously, 0 on success, a negative ECM_E* code of ecm_hip.h on a
 * bad argument (ecm_error_string names it) or the positive hipError_t of a failed launch.  Forward only.
 *
 * ---- The map (OpenCV's initUndistortRectifyMap, evaluated in double) ----
 * For output pixel (u, v), u = 0..Wo-1, v = 0..Ho-1, with params = ecmr_rectify_map_params() doubles
 *     iR[0..8] (row-major, (P[:, :3] R)^-1),  fx fy cx cy,  k1 k2 p1 p2 k3 k4 k5 k6        (coefficients not given: 0)
 * every line below is evaluated in IEEE fp64, one operation per product, sum and quotient, in the order the parentheses give,
 * without fused multiply-adds:
 *     X = (iR0 u + iR1 v) + iR2      Y = (iR3 u + iR4 v) + iR5      W = (iR6 u + iR7 v) + iR8
 *     x = X / W      y = Y / W
 *     x2 = x x       y2 = y y        r2 = x2 + y2      r4 = r2 r2      r6 = r4 r2      xy2 = 2 (x y)
 *     radial = (((1 + k1 r2) + k2 r4) + k3 r6) / (((1 + k4 r2) + k5 r4) + k6 r6)
 *     xd = x radial + (p1 xy2 + p2 (r2 + 2 x2))
 *     yd = y radial + (p1 (r2 + 2 y2) + p2 xy2)
 *     mx = fx xd + cx                my = fy yd + cy
 * and map[0][v][u] = (float)mx, map[1][v][u] = (float)my: each rounded once to fp32.  The pinhole model with rational radial and
 * tangential distortion only: no fisheye, thin-prism or tilt terms.  A pixel whose W is 0 gets whatever IEEE gives (inf or NaN):
 * ecmr_remap_pair_fwd treats a non-finite map entry as outside.
 *
 * ---- The remap (bilinear, in fp32) ----
 * For output pixel (u, v) of image b and view (left / right) with (mx, my) = that view's map entry:
 *     x0 = floorf(mx)   ax = mx - x0     y0 = floorf(my)   ay = my - y0                    (both differences are exact)
 *     t00 t01 t10 t11 = the source at (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) as fp32, per channel; a tap whose column is
 *       outside 0..W-1 or whose row is outside 0..H-1 is `border`
 *     top = t00 + ax (t01 - t00)     bot = t10 + ax (t11 - t10)     s = top + ay (bot - top)
 *       each product, sum and difference one fp32 operation, without fused multiply-adds
 *     out[b][c][v][u] = (s / 255 - mean[c]) / std[c]       IEEE fp32 divisions: the expression of ecm_frame_prep, so a map of
 *       integer coordinates (ax = ay = 0, s = t00) reproduces its planes bit for bit
 *     image[b][c][v][u] = s / 255                          (left view only)
 *     mask[b][v][u] = 1 where mx and my are finite and all four taps lie inside the source (0 <= x0 <= W-2, 0 <= y0 <= H-2), else
 *       0: a coordinate exactly on the last column or row is NOT inside, although its outer taps have weight 0
 *   A non-finite mx or my: s = border in every channel, mask 0.  `border`, like the source, is in 0..255 units.
 */
#ifndef ECM_RECTIFY_H
#define ECM_RECTIFY_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Both queries need no GPU.  ecmr_rectify_map_params: the doubles of `params` (21).  ecmr_tile_width: the output columns one
 * workgroup of either kernel covers (64); rows of other widths end in a partial workgroup. */
int ecmr_rectify_map_params(void);
int ecmr_tile_width(void);

/* map [2,Ho,Wo] fp32 from params (device, fp64), one launch.  ECM_EINVAL, before any device work: a null pointer, Ho or Wo < 1,
 * map equal to params.  ECM_EUNSUP, before any launch: Ho * Wo >= 2^31 or Ho > 262140. */
int ecmr_rectify_map_fwd(const double* params, float* map, int Ho, int Wo, void* stream);

/* Both views of B pairs in ONE launch (the view and the image are the grid's z).
 *   left_raw, right_raw: unsigned char [B,H,W,3] (src_is_u8 != 0) or float [B,3,H,W] holding 0..255 (src_is_u8 == 0).
 *   map_left, map_right: fp32 [2,Ho,Wo] shared by the batch (map_per_image == 0) or [B,2,Ho,Wo] (map_per_image != 0).
 *   left, right: fp32 [B,3,Ho,Wo].  image (fp32 [B,3,Ho,Wo]), mask_left, mask_right (unsigned char [B,Ho,Wo]) may each be NULL.
 *   mean3, std3: HOST arrays of three floats;  border: finite.
 * A thread owns four consecutive output columns and stores 16 bytes per plane where Wo is a multiple of 4 and every map and
 * output pointer is 16-byte aligned; otherwise every pixel is loaded and stored on its own.  No atomics, no LDS, no scratch:
 * bit-reproducible, and an image's planes do not depend on the rest of the batch.
 * ECM_EINVAL, before any device work: a null source, map, left, right, mean3 or std3; B, H, W, Ho or Wo < 1; border not finite;
 * std3[c] == 0 or a non-finite mean3[c] or std3[c]; an output equal to, or overlapping, an input or another output.
 * ECM_EUNSUP, before any launch: B * max(H * W, Ho * Wo) >= 2^31, H or W > 2^24, B > 32767 or Ho > 1048560. */
int ecmr_remap_pair_fwd(const void* left_raw, const void* right_raw, int src_is_u8, const float* map_left, const float* map_right,
                        int map_per_image, float* left, float* right, float* image, unsigned char* mask_left,
                        unsigned char* mask_right, int B, int H, int W, int Ho, int Wo, const float* mean3, const float* std3,
                        float border, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_RECTIFY_H */
