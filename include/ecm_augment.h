/*
 * ecm_augment.h -- the augmentation entries of libecm_hip.so: the photometric training transform of the reference's KITTI loader
 * (cmf/loader/KITTI.py:144-191: torchvision's ColorJitter on a PIL image, a PCA "lighting" shift, a clamp and the normalisation)
 * inside the decode of a packed frame, and the colour jitter alone on resident uint8 images.  DESIGN.md section 37.
 *
 * A ninth header beside ecm_hip.h, ecm_geometry.h, ecm_rectify.h, ecm_temporal.h, ecm_motion.h, ecm_volume.h, ecm_mesh.h and
 * ecm_color.h, with its own prefix (ecma_).  The conventions are ecm_hip.h's: plain pointers and ints, every pointer a DEVICE
 * pointer the caller owns unless it says HOST, `stream` a hipStream_t passed as void* (NULL = default stream), work enqueued
 * asynchronously, 0 on success, a negative ECM_E* code of ecm_hip.h on a bad argument (ecm_error_string names it) or the positive
 * hipError_t of a failed launch.  Every refusal happens before any HIP call.
 *
 * A VIEW is one RGB image of n = rows * columns pixels.  Its jitter is up to four operations, each on the uint8 RGB result of the
 * one before it, in the order the view's `order` gives: four ints, the distinct codes present first and -1 behind them;
 *   0 brightness, 1 contrast, 2 saturation, 3 hue.
 * factors holds three floats per view (brightness, contrast, saturation; read only where the operation is present), hue_shift one
 * int in 0..255.  Every fp32 operation below is rounded on its own: no fused multiply-add.
 *
 *   L (gray)      (19595 R + 38470 G + 7471 B + 0x8000) >> 16, in integers.
 *   blend(d,a,f)  t = d + f * (a - d) in fp32;  0 where t <= 0, 255 where t >= 255, else t truncated.  (For 0 <= f <= 1 the
 *                 bounds never bind.)
 *   brightness    blend(0, a, f) per channel.
 *   contrast      m = floor((2 S + n) / (2 n)) in integers, S the sum of L over the view AS IT STANDS when contrast is reached;
 *                 blend(m, a, f) per channel.
 *   saturation    blend(L, a, f) per channel, L the pixel's own.
 *   hue           RGB -> HSV, h = (h + hue_shift) mod 256, HSV -> RGB; made for a shift of 0 too (it is not the identity).
 *     RGB -> HSV  v = max.  max == min: h = s = 0.  Else in fp32 cr = max - min, s = cr / max, rc = (max - r) / cr and likewise
 *                 gc, bc;  h = bc - gc (fp32) where r is the maximum, else 2.0 + rc - bc (fp64) where g is, else
 *                 4.0 + gc - rc (fp64), rounded to fp32;  h = (float) fmod(h / 6.0 + 1.0, 1.0) in fp64;
 *                 uh = clip8((int)(h * 255.0)), us = clip8((int)(s * 255.0)), both products in fp64.
 *     HSV -> RGB  s == 0: r = g = b = v.  Else in fp32 fs = s / 255, f = h * 6 / 255, i = floor(f), f = f - i,
 *                 p = floor(v * (1 - fs) + 0.5), q = floor(v * (1 - fs * f) + 0.5), t = floor(v * (1 - fs * (1 - f)) + 0.5), each
 *                 clipped to 0..255;  i mod 6 = 0: (v,t,p), 1: (q,v,p), 2: (p,v,t), 3: (p,q,v), 4: (t,p,v), 5: (v,p,q).
 *
 * These are Pillow's ImageEnhance.Brightness / Contrast / Color and its HSV conversions, byte for byte (tests/golden/g13_jitter.npz).
 *
 * Two launches.  Where some view of a launch chunk has contrast, a reduction launch runs first: one workgroup of 256 threads per
 * tile of ecma_jitter_tile() pixels of a view applies the operations in front of contrast and writes the integer sum of L over
 * its tile to scratch[view * tiles + tile] (uint32; tiles = ceil(n / ecma_jitter_tile())); a view without contrast writes
 * nothing.  The apply launch has the same grid; a workgroup of a view with contrast adds that view's partials (integers: any order
 * gives the same sum), forms m and runs the operations.  No atomics, no zeroing pass, no float sums: bit-reproducible, and a
 * view does not depend on the others of the batch.
 */
#ifndef ECM_AUGMENT_H
#define ECM_AUGMENT_H

#include "ecm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The pixels of one reduction tile: 2048 (256 threads, 8 pixels each).  No GPU needed. */
int ecma_jitter_tile(void);

/* Bytes of scratch the two entries below need for `views` views of rows x cols pixels: views * ceil(rows * cols / tile) * 4.
 * 0 for sizes the entries refuse (a count below 1, rows > 65535, rows * cols > 2^24).  No GPU needed. */
long long ecma_jitter_scratch_bytes(int views, int rows, int cols);

/* The jitter of N resident views: images, out uint8 [N,H,W,3].  factors, order and hue_shift are HOST arrays of N * 3 floats,
 * N * 4 ints and N ints.  scratch: ecma_jitter_scratch_bytes(N, H, W) bytes, 4-byte aligned, contents irrelevant before and
 * after.  At most 64 views per launch; more are chunked.
 * ECM_EINVAL: a null images, out, factors, order, hue_shift or scratch; N, H or W < 1; out equal to images; an order that is not
 * distinct codes 0..3 followed by -1s; a hue_shift outside 0..255.  ECM_EUNSUP: H > 65535 or H * W > 2^24.  ECM_ESCRATCH:
 * scratch_bytes below the size query. */
int ecma_color_jitter_fwd(const unsigned char* images, unsigned char* out, int N, int H, int W, const float* factors, const int* order,
                          const int* hue_shift, void* scratch, long long scratch_bytes, void* stream);

/* ecm_frame_prep_packed's window decode (mode 0 without a tail) with the training transform of KITTI.py:144-191 in it.  rgb6 uint8
 * [B,H,W,6] (left RGB, right RGB) and disp_in fp16 (disp_is_half != 0) or fp32 [B,H,W];  sample b's window is rows crop_y0[b] ..
 * + th, columns crop_x0[b] .. + tw (HOST arrays of B ints).  Its two views are view 2b (left) and 2b + 1 (right) of the HOST
 * arrays factors [B,2,3], order [B,2,4], hue_shift [B,2] and pca [B,2,3].  Per view, with u the jittered uint8 window, in fp32:
 *     x = u / 255;   x = x + pca[c];   x = min(max(x, 0), 1);   out = (x - mean3[c]) / std3[c]     (IEEE division)
 * left, right [B,3,th,tw] fp32 get `out`, image [B,3,th,tw] (may be NULL) the left view's clamped x (KITTI.py:189), and disp
 * [B,th,tw] fp32 the window of disp_in, widened.  mean3, std3: HOST arrays of 3 floats.  scratch: ecma_jitter_scratch_bytes(2 * B,
 * th, tw) bytes.  At most 32 samples per launch; more are chunked.
 * ECM_EINVAL: a null rgb6, disp_in, left, right, disp, crop_y0, crop_x0, factors, order, hue_shift, pca, mean3, std3 or scratch;
 * B, H, W, th or tw < 1; a window outside its frame; an order or a hue_shift as above.  ECM_EUNSUP: th > 65535 or th * tw > 2^24.
 * ECM_ESCRATCH: scratch_bytes below the size query. */
int ecma_frame_prep_jitter_fwd(const unsigned char* rgb6, const void* disp_in, int disp_is_half, float* left, float* right, float* disp,
                               float* image, int B, int H, int W, const int* crop_y0, const int* crop_x0, int th, int tw,
                               const float* factors, const int* order, const int* hue_shift, const float* pca, const float* mean3,
                               const float* std3, void* scratch, long long scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_AUGMENT_H */
