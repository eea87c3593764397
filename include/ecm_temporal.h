/*
 * ecm_temporal.h -- the temporal entries of libecm_hip.so: a disparity map carried to the next frame by a known camera motion,
 * and its fusion with that frame's own estimate.
 *
 * A fourth header beside ecm_hip.h, ecm_geometry.h and ecm_rectify.h, with its own prefix (ecmt_).  The conventions are
 * ecm_hip.h's: plain pointers and ints, every pointer a DEVICE pointer the caller owns, `stream` a hipStream_t passed as void*
 * (NULL = default stream), work enqueued asynchronously, 0 on success, a negative ECM_E* code of ecm_hip.h on a bad argument
 * (ecm_error_string names it) or the positive hipError_t of a failed launch.
 *
 * Definition of the warp.  M_b is a 4x4 fp64 matrix, 16 doubles per image, row-major ([B,4,4], m_per_image != 0), or one matrix
 *   shared by the batch ([4,4], m_per_image == 0).  For a rigid motion T between two left-camera frames and the disparity-to-
 *   depth matrices Q, Q_out of ecm_geometry.h it is M = Q_out^-1 T Q: Q is projective, so the motion acts on (x, y, d, 1) as one
 *   matrix.  For pixel (x, y) of image b with disparity d = disp[b,y,x]:
 *     [a b c w]^T = M_b * [x y d 1]^T,    row r:  ((M[r][0] * x + M[r][1] * y) + M[r][2] * d) + M[r][3]
 *   every product and sum one IEEE fp64 operation, in that order, without fused multiply-adds (ecm_geometry.h's row).
 * Usable pixel (ecm_geometry.h's rule).  All of: d finite;  valid[b,y,x] != 0 (an unsigned char plane; NULL: all ones);
 *   min_disp < d <= max_disp, compared in fp32 (max_disp may be +inf; min_disp must be finite);  w finite and non-zero.
 * Candidate.  A usable pixel for which u = a / w, v = b / w (fp64 divisions) and dn = (float)(c / w) (rounded once to fp32) are
 *   finite, dn > 0, 0 <= u <= W-1 and 0 <= v <= H-1, compared in fp64: the in-view rule of ecm_disp_splat_fwd in two dimensions.
 * Landing sites of a candidate, with x0 = floor(u), y0 = floor(v):
 *   footprint 0 ("cover"):   (x0, y0); also column x0 + 1 iff u > x0, and also row y0 + 1 iff v > y0: one, two or four sites,
 *                            none outside the image (u > x0 implies x0 < W-1, v > y0 implies y0 < H-1).
 *   footprint 1 ("nearest"): the one site (floor(u + 0.5), floor(v + 0.5)), each clamped to W-1 / H-1.
 * Winner.  Per landing site the candidate with the largest 64-bit key: the high 32 bits are the bits of dn -- positive and finite,
 *   so their unsigned order is the float order -- the low 32 bits the source's linear index y * W + x.  The largest new disparity
 *   wins (the nearest surface hides what lies behind it), among equal disparities the larger source index.  Every key is at
 *   least 2^32; the key 0 is the hole: nothing landed.
 * Outputs.  out [B,H,W] fp32: the winner's dn bit for bit, +0.0 for a hole.  src [B,H,W] int (may be NULL): the winner's linear
 *   index, -1 for a hole.  attrs_out [B,C,H,W] fp32: attrs[b,c] at the winner's source pixel bit for bit, +0.0 for a hole.
 */
#ifndef ECM_TEMPORAL_H
#define ECM_TEMPORAL_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The z-buffered forward warp.  scratch: ecmt_disparity_warp_scratch_bytes(B, H, W) bytes, one 8-byte key per pixel of the
 * batch, 8-byte aligned; the entry clears it itself.  On `stream`: hipMemsetAsync of the keys; a scatter pass in tiles of
 * consecutive pixels of one image, which reads disp (and valid) coalesced and issues one to four 64-bit integer atomic maxima
 * per candidate on the keys in global memory; a resolve pass, which reads the keys coalesced, decodes them, gathers the C
 * attribute planes at the winner's source and stores out, src and attrs_out.  The only atomics are integer maxima and no
 * workgroup waits for another: the result does not depend on the order of arrival, is bit-reproducible, and image b's planes do
 * not depend on the other images.
 * Both queries need no GPU; the scratch query answers 0 for a shape the entry refuses.  ECM_EINVAL, before any device work: a
 * null disp, M, out or scratch, B, H or W < 1, min_disp not finite, max_disp NaN or below min_disp, C outside
 * 0..ecmt_disparity_warp_max_attributes(), attrs or attrs_out null with C > 0, out, src, attrs_out or scratch equal to disp,
 * valid, M or attrs.  ECM_EUNSUP, before any launch: footprint outside {0, 1}, H * W >= 2^31, or
 * B * ceil(H * W / 2048) >= 2^24 (the launch indexes one tile of 2048 pixels per workgroup).  ECM_ESCRATCH: scratch_bytes too
 * small. */
int       ecmt_disparity_warp_max_attributes(void);
long long ecmt_disparity_warp_scratch_bytes(int B, int H, int W);
int ecmt_disparity_warp_fwd(const float* disp, const unsigned char* valid, const double* M, int m_per_image, const float* attrs,
                            int C, float* out, int* src, float* attrs_out, void* scratch, long long scratch_bytes, int B, int H,
                            int W, float min_disp, float max_disp, int footprint, void* stream);

/* The per-pixel fusion of a frame's own estimate (disp, var) with the state warped into it (prev, prev_var), n elements each,
 * one launch.  Every operation is one fp32 operation in the stated order, without fused multiply-adds.
 *   A measurement exists iff disp is finite and > 0 and var is finite and > 0.
 *   A prediction exists iff prev > 0 and prev_var is finite and > 0.
 *   The predicted variance s = prev_var + process_noise, or, with prev_source (may be NULL; the disparity the warp's winner had
 *     before the warp), s = (((prev_var * r) * r) * r) * r + process_noise with r = prev / prev_source: the first-order
 *     propagation of the variance for a motion along the optical axis, and only that.
 *   Both exist and e * e <= (gate * gate) * (s + var), e = disp - prev:  K = s / (s + var);  fused = prev + K * e;
 *     fused_var = (1 - K) * s;  age = prev_age + 1.
 *   Both exist and the gate fails, or only a measurement exists:  (disp, var, 1).
 *   Only a prediction exists:  (prev, s, prev_age) where coast != 0, else (0, 0, 0).     Neither exists:  (0, 0, 0).
 * prev_age (int, may be NULL: all zeros) and age are ints.  Elementwise: an output may be the input of the same type.
 * ECM_EINVAL, before any device work: a null disp, var, prev, prev_var, fused, fused_var or age, n < 1, gate or process_noise
 * not finite or negative. */
int ecmt_disparity_fuse_fwd(const float* disp, const float* var, const float* prev, const float* prev_var, const int* prev_age,
                            const float* prev_source, float* fused, float* fused_var, int* age, long long n, float gate,
                            float process_noise, int coast, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_TEMPORAL_H */
