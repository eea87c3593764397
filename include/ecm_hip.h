/*
 * ecm_hip.h -- C ABI of libecm_hip.so: the MI355X (gfx950) hot path of the
 * Explicit-Context-Mapping stereo network (reference: cmf/models/cmfsm.py).
 *
 * Conventions (all entry points):
 *   - plain pointers and ints only; every pointer is a DEVICE pointer that the
 *     caller owns (borrowed; kernels never allocate, free or synchronise);
 *   - tensors are contiguous fp32, NCHW / NCDHW exactly as the reference holds them;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); work is
 *     enqueued asynchronously on it;
 *   - return 0 on success, a negative ECM_E* code on a bad argument, or the positive
 *     hipError_t of a failed launch; no exceptions cross the ABI;
 *   - which negative code: ECM_EINVAL for a null pointer (unless the entry says it may be NULL) and for a size, count or extent
 *     that is zero or negative, and for arguments that contradict each other (a window outside its frame); ECM_EUNSUP for a
 *     positive value that the kernels are not built for, and for ANY value of a stride, dilation, kernel size (kd, k; kh, kw of
 *     the convolutions), head count, variant or mode outside the set its entry names, zero and negative ones included: these
 *     select a kernel, they do not size one; ECM_ESCRATCH for a scratch buffer below the entry's size query.  Every refusal
 *     is answered on the host, before any device work, and a size query answers 0 for the sizes its entry refuses
 *     (tests/test_abi_refusals.py holds all of this for every entry, without a device);
 *   - re-entrant; the only process-wide state is the sticky asynchronous-error word (ecm_async_status) and the
 *     GroupNorm cluster mode (ecm_gn3d_cluster_mode), both documented below.
 *
 * Each function cites the reference interface (file:line under the reference repo)
 * it replaces; INTEGRATION.md shows the ctypes binding a maintainer would add.
 */
#ifndef ECM_HIP_H
#define ECM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ECM_EINVAL   (-1)   /* bad shape / null pointer */
#define ECM_EUNSUP   (-2)   /* shape outside what the kernels are built for */
#define ECM_ESCRATCH (-3)   /* caller-provided scratch too small */
#define ECM_EASYNC   (-4)   /* an EARLIER asynchronous launch failed on the device (sticky; see ecm_async_status) */

/* Library / build info. */
int         ecm_abi_version(void);            /* bumps on any signature change */
const char* ecm_error_string(int code);       /* for both ECM_E* and hipError_t codes */

/* ---- a1: cost volume (cmfsm.py:667-682; == cat_d matchshifted, cmfsm.py:88-108) ------------
 * cost[b, c,   d, y, x] = L[b,c,y,x]     if x >= d else 0
 * cost[b, C+c, d, y, x] = R[b,c,y,x-d]   if x >= d else 0
 * L,R: [B,C,h,w]; cost: [B,2C,D,h,w].  fwd writes every element (no pre-zeroing needed). */
int ecm_costvol_concat_fwd(const float* L, const float* R, float* cost,
                           int B, int C, int h, int w, int D, void* stream);
/* gL[b,c,y,x] = sum_{d<=x} gcost[b,c,d,y,x];  gR[b,c,y,x'] = sum_{d, x'+d<w} gcost[b,C+c,d,y,x'+d] */
int ecm_costvol_concat_bwd(const float* gcost, float* gL, float* gR,
                           int B, int C, int h, int w, int D, void* stream);

/* ---- a8: soft-argmin over D (cmfsm.py:703-706 + disparityregression 111-123) -----------------
 * Fused three-head form: logits_k = sum_{j<=k} c_j (cmfsm.py:725,748), disp[k] = sum_d softmax_d(logits_k)*d.
 * c: nheads pointers' worth of [B,D,h*w] raw classifier outputs packed as c[head] = c0 + head*head_stride.
 * disp: [nheads,B,h*w].  nheads in 1..3, else ECM_EUNSUP; head_stride >= 0, else ECM_EINVAL: so for every entry that takes them. */
int ecm_softargmin_heads_fwd(const float* c0, long long head_stride, float* disp,
                             int nheads, int B, int D, int hw, void* stream);
/* gc[head] (same packing as c) from gdisp [nheads,B,hw]; recomputes the softmax. */
int ecm_softargmin_heads_bwd(const float* c0, long long head_stride, const float* gdisp, float* gc0,
                             int nheads, int B, int D, int hw, void* stream);
/* ABI 8: ecm_softargmin_heads_fwd that also writes lse[k,b,p] = max_d logits_k + ln sum_d exp(logits_k - max), [nheads,B,hw]:
 * softmax_d(logits_k) = exp(logits_k[d] - lse).  disp is bit-identical to ecm_softargmin_heads_fwd's. */
int ecm_softargmin_heads_lse_fwd(const float* c0, long long head_stride, float* disp, float* lse,
                                 int nheads, int B, int D, int hw, void* stream);
/* disparityregression.forward alone (cmfsm.py:120-123): out[b,p] = sum_d x[b,d,p]*d */
int ecm_disparity_regression_fwd(const float* x, float* out, int B, int D, int hw, void* stream);

/* ---- a9: NN-upsample x scale + 9-neighbour weighted sum (cmfsm.py:709-723, 730-744, 755-769) --
 * out[k,b,Y,X] = sum_n w9[b,n,Y,X] * s * d[k,b,Y/s+dy_n,X/s+dx_n]   (0 outside), n order: c,l,r,t,b,lt,rt,lb,rb
 * d: [nheads,B,h,w]; w9: [B,9,H,W] (H=h*s, W=w*s); out: [nheads,B,H,W]. */
int ecm_aggregate9_fwd(const float* d, const float* w9, float* out,
                       int nheads, int B, int h, int w, int s, void* stream);
int ecm_aggregate9_bwd(const float* d, const float* w9, const float* gout, float* gd, float* gw9,
                       int nheads, int B, int h, int w, int s, void* stream);
/* ABI 8: per-pixel uncertainty of ecm_aggregate9_fwd's output.  The HR pixel's distribution is the
 * mixture p(d) = sum_n w9[n] p_n(d) / sum_n w9[n] over the neighbours ecm_aggregate9_fwd does not skip, p_n the LR softmax of
 * cell+n over d < D (c0 / head_stride as in ecm_softargmin_heads_fwd, lse from ecm_softargmin_heads_lse_fwd).
 * stats: [nheads,3,B,H,W] = s * standard deviation of p about its own mean (full-resolution pixels), max_d p, entropy (nats). */
int ecm_aggregate9_stats_fwd(const float* c0, long long head_stride, const float* lse, const float* w9, float* stats,
                             int nheads, int B, int D, int h, int w, int s, void* stream);
/* ABI 9: the modal disparity of the same mixture p, L = D levels spaced u = s full-resolution pixels.
 * radius >= 0 is in full-resolution pixels and a multiple of s (else ECM_EINVAL); r = radius / s.
 * modal: [nheads,3,B,H,W] = (mode, mass, index):
 *   index = s * D*, D* = argmax_d p(d), the lowest d winning an exact tie (a float plane of exact integers);
 *   mass  = sum_{d in Wn} p(d), clamped to <= 1, Wn = {d : |d - D*| <= r, 0 <= d < D};
 *   mode  = s * (D* + sum_{Wn} p(d) (d - D*) / sum_{Wn} p(d)), formed centred on D*.
 * The border factor sum_valid w9 of the head's output is not applied (as for std above).  A NaN logit in a pixel's valid
 * neighbourhood makes all three planes NaN there.  Any D works (the levels are staged through LDS in chunks of at most 48);
 * ECM_EUNSUP for nheads outside 1..3 or B > 65535.  Writes only `modal`: the disparity is ecm_aggregate9_fwd's. */
int ecm_aggregate9_mode_fwd(const float* c0, long long head_stride, const float* lse, const float* w9, float* modal,
                            int nheads, int B, int D, int h, int w, int s, int radius, void* stream);

/* ---- a3: eight-related context-mapping weights (cmfsm.py:431-593, 304-358, 391-428) ----------
 * lr: [B,32,h,w]; hr: [B,32,H,W]; W0 [32,66], W1 [16,32], W2 [8,16], W3 [1,8] (1x1 conv weights, no bias);
 * w9: [B,9,H,W] softmax planes in the reference's return order.
 * scratch: >= ecm_weights9_scratch_bytes(B,h,w) bytes of device memory. */
long long ecm_weights9_scratch_bytes(int B, int h, int w);
int ecm_weights9_fwd(const float* lr, const float* hr, const float* W0, const float* W1, const float* W2,
                     const float* W3, float* w9, void* scratch, long long scratch_bytes,
                     int B, int h, int w, int s, void* stream);
/* Gradients of all inputs from gw9 [B,9,H,W].  gW = [gW0(2112) | gW1(512) | gW2(128) | gW3(8)] floats. */
long long ecm_weights9_bwd_scratch_bytes(int B, int h, int w, int s);
int ecm_weights9_bwd(const float* lr, const float* hr, const float* W0, const float* W1, const float* W2,
                     const float* W3, const float* w9, const float* gw9,
                     float* glr, float* ghr, float* gW, void* scratch, long long scratch_bytes,
                     int B, int h, int w, int s, void* stream);

/* ---- a4: six-related context mapping (cmfsm_sub_8.py:440-572; same text in cmfsm_sub_16.py, cm_sub_4/8/16.py) and the
 * general form of a3.  variant 0: eight_related (9 planes, softmax; == ecm_weights9_fwd); variant 1: six_related on the
 * reference image (5 planes c,r,l,t,b; zero padding; extra LeakyReLU; output softmax*logit); variant 2: six_related on
 * the target image (3 planes c,r,l).  out: [B,N,H,W], N = 9/5/3.  Any even scale s for variants 1 and 2; variant 0 is built for
 * s = 4 (ECM_EUNSUP otherwise, as for an odd s or a variant outside 0..2).  scratch: ecm_weights9_scratch_bytes(B,h,w) bytes. */
int ecm_context_weights_fwd(const float* lr, const float* hr, const float* W0, const float* W1, const float* W2,
                            const float* W3, float* out, void* scratch, long long scratch_bytes,
                            int B, int h, int w, int s, int variant, void* stream);

/* Backward of ecm_context_weights_fwd for any variant and any scale with s % 4 == 0.  out_saved = the forward output
 * (used by variant 0; variants 1/2 recompute their logits).  gW = [gW0(2112) | gW1(512) | gW2(128) | gW3(8)] floats.
 * s <= 0: ECM_EINVAL; any other s outside {4, 8, 16}: ECM_EUNSUP, and the size query answers 0. */
long long ecm_context_weights_bwd_scratch_bytes(int B, int h, int w, int s, int variant);
int ecm_context_weights_bwd(const float* lr, const float* hr, const float* W0, const float* W1, const float* W2,
                            const float* W3, const float* out_saved, const float* gout,
                            float* glr, float* ghr, float* gW, void* scratch, long long scratch_bytes,
                            int B, int h, int w, int s, int variant, void* stream);

/* ---- a10: volume mapping head (cmfsm_sub_16.py:767-801 [+804-848], cm_sub_8.py:765-800), fused: NN-upsample of the LR
 * logits in D,H,W, 5-neighbour spatial fuse with m5 [B,5,H,W] (c,r,l,t,b), three target-weight volumes built from
 * mt3 [B,3,H,W] (c,r,l) shifted by the disparity, +-s fuse along D, softmax over D = Dl*s, regression.
 * c: raw classifier outputs [nheads][B,Dl,h,w] (head k uses c_0+...+c_k); disp: [nheads,B,H,W]. */
int ecm_volume_mapping_fwd(const float* c0, long long head_stride, const float* m5, const float* mt3, float* disp,
                           int nheads, int B, int Dl, int h, int w, int s, void* stream);
/* ABI 8: the same kernel body, which also writes stats [nheads,3,B,H,W] = standard deviation (pixels), peak and entropy
 * (nats) of the softmax over D whose mean is disp; disp is bit-identical to ecm_volume_mapping_fwd's. */
int ecm_volume_mapping_stats_fwd(const float* c0, long long head_stride, const float* m5, const float* mt3, float* disp,
                                 float* stats, int nheads, int B, int Dl, int h, int w, int s, void* stream);
/* ABI 9: the modal disparity of that softmax p over the L = Dl*s fused logits, u = 1, r = radius >= 0.
 * modal: [nheads,3,B,H,W] = (mode, mass, index): index = D* = argmax_D p(D), the lowest D winning an exact tie;
 * mass = sum_{|D - D*| <= r} p(D) <= 1; mode = D* + sum_W p(D) (D - D*) / sum_W p(D), centred on D*.  A NaN logit in the pixel's
 * support makes all three NaN.  The parent's operands and refusals; writes only `modal`. */
int ecm_volume_mapping_mode_fwd(const float* c0, long long head_stride, const float* m5, const float* mt3, float* modal,
                                int nheads, int B, int Dl, int h, int w, int s, int radius, void* stream);
/* Gradients of c (same packing), m5 and mt3 from gdisp [nheads,B,H,W]; s must be a power of two <= 64.  Deterministic:
 * every sum is taken in a fixed order (per-row partial sums in `scratch`, gathered by a second kernel; no float atomics),
 * every output element is written exactly once. */
long long ecm_volume_mapping_bwd_scratch_bytes(int nheads, int B, int Dl, int h, int w, int s);
int ecm_volume_mapping_bwd(const float* c0, long long head_stride, const float* m5, const float* mt3, const float* gdisp,
                           float* gc0, float* gm5, float* gmt3, void* scratch, long long scratch_bytes,
                           int nheads, int B, int Dl, int h, int w, int s, void* stream);

/* ---- a11: trilinear head (bilinear_cmf.py:447-471), fused: F.interpolate(trilinear, align_corners=False) of the LR
 * logits to [Do,H,W], softmax over Do, regression.  c as above (cumulative over heads); disp: [nheads,B,H,W]. */
int ecm_trilinear_softargmin_fwd(const float* c0, long long head_stride, float* disp,
                                 int nheads, int B, int Dl, int h, int w, int Do, int H, int W, void* stream);
/* ABI 8: with stats [nheads,3,B,H,W] as ecm_volume_mapping_stats_fwd; disp bit-identical to ecm_trilinear_softargmin_fwd's. */
int ecm_trilinear_softargmin_stats_fwd(const float* c0, long long head_stride, float* disp, float* stats,
                                       int nheads, int B, int Dl, int h, int w, int Do, int H, int W, void* stream);
/* ABI 9: modal [nheads,3,B,H,W] = (mode, mass, index) of the softmax over the Do interpolated logits, defined as for
 * ecm_volume_mapping_mode_fwd (L = Do, u = 1, r = radius >= 0); writes only `modal`. */
int ecm_trilinear_softargmin_mode_fwd(const float* c0, long long head_stride, float* modal, int nheads, int B, int Dl,
                                      int h, int w, int Do, int H, int W, int radius, void* stream);
/* Deterministic (per-pixel plane gradients in `scratch`, then separable fixed-order reductions along x and y). */
long long ecm_trilinear_softargmin_bwd_scratch_bytes(int nheads, int B, int Dl, int h, int w, int H, int W);
int ecm_trilinear_softargmin_bwd(const float* c0, long long head_stride, const float* gdisp, float* gc0,
                                 void* scratch, long long scratch_bytes,
                                 int nheads, int B, int Dl, int h, int w, int Do, int H, int W, void* stream);

/* ---- a5-a7: 3-D aggregation (cmfsm.py:49-58 convbn_3d, 240-303 hourglass, 604-634) ----------
 * Weights are taken in the reference (checkpoint) layouts and repacked on device by the *_pack calls. */

/* Repack Conv3d weight [Co,Ci,3,3,3] -> kernel layout [27][Ci][CoP] (CoP = Co rounded up to 32).
 * flip_transpose != 0 packs the data-gradient operator of a stride-1 conv instead (taps reversed, Ci/Co
 * swapped: a conv with Cin'=Co, Cout'=Ci), so dgrad runs on ecm_conv3d_k3_fwd too. */
long long ecm_conv3d_packed_floats(int Ci, int Co);
int ecm_conv3d_pack_weight(const float* w, float* packed, int Co, int Ci, int flip_transpose, void* stream);

/* y[b,co,od,oh,ow] = sum w[co,ci,kd,kh,kw] x[b,ci,od*st+kd-1,oh*st+kh-1,ow*st+kw-1]; k=3, pad=1, st in {1,2}.
 * x: [B,Ci,D,H,W]; y: [B,Co,Do,Ho,Wo] with Do=(D-1)/st+1 etc.  Ci % 4 == 0; 1 <= Co <= 64 (ECM_EUNSUP; Ci, Co <= 0: ECM_EINVAL). */
int ecm_conv3d_k3_fwd(const float* x, const float* wpacked, float* y,
                      int B, int Ci, int Co, int D, int H, int W, int stride, void* stream);

/* The same stride-1 convolution by Winograd F(2x2,3x3) in the (h,w) plane, direct along depth (conv_wino.hip): 2.25x fewer
 * multiplies, fp32 throughout (transforms add/subtract/halve only; results differ from the direct kernel by fp32 rounding).
 * kd = 3: Conv3d 3x3x3, x [B,Ci,D,H,W] -> y [B,Co,D,H,W];  kd = 1: Conv2d 3x3 applied to each of the D planes (D = 1 for
 * a plain image; D = d*d phase planes of a dilation-d layer, see models.feature_extraction).  Any Ci, Co (32 output
 * channels per workgroup; more go to a second grid dimension).  Weights: reference layout [Co,Ci,kd,3,3], transformed and
 * packed by ecm_conv_wino_pack_weight (flip_transpose != 0: the data-gradient operator, Cin' = Co, Cout' = Ci; size query
 * with the swapped counts). */
long long ecm_conv_wino_packed_floats(int Ci, int Co, int kd);
int ecm_conv_wino_pack_weight(const float* w, float* packed, int Co, int Ci, int kd, int flip_transpose, void* stream);
/* Both layouts in one launch: packed[0 .. packed_floats(Ci,Co,kd)) = the forward layout, followed by the data-gradient layout
 * (packed_floats(Co,Ci,kd) floats) -- what a training step needs of every layer (forward now, backward later). */
int ecm_conv_wino_pack_weight2(const float* w, float* packed, int Co, int Ci, int kd, void* stream);
int ecm_conv_wino_fwd(const float* x, const float* upacked, float* y, int B, int Ci, int Co, int D, int H, int W, int kd,
                      void* stream);
/* out = ((a + b) + c) + d elementwise over n floats, c and d optional (NULL): the gradient accumulation of a tensor with
 * several consumers in one pass (cmfsm.py:686-693: cost0 feeds the first hourglass and three residual adds) instead of
 * autograd's chain of binary adds.  d only together with c (d without c: ECM_EINVAL).  16-byte aligned pointers (ECM_EUNSUP
 * otherwise); out may alias an input. */
int ecm_sum_n(const float* a, const float* b, const float* c, const float* d, float* out, long long n, void* stream);
/* out [planes,H,W] = small [planes,Hs,Ws] on the even positions, 0 elsewhere: the data gradient of a 1x1 / stride-2 projection
 * (the encoder's downsample layers) once W^T gy exists on the coarse grid. */
int ecm_zero_insert2d(const float* small, float* out, long long planes, int H, int W, int Hs, int Ws, void* stream);

/* y = conv(x) + addend, addend shaped like y and added in the kernel's epilogue: with the data-gradient weights this is
 * autograd's accumulation at a skip connection (gx = dgrad(gy) + g_skip; BasicBlock cmfsm.py:76-85, dres1 612-613, the
 * hourglass / classifier inputs 636-660) without the separate elementwise pass.  y may not alias addend. */
int ecm_conv_wino_fwd_add(const float* x, const float* upacked, const float* addend, float* y, int B, int Ci, int Co, int D,
                          int H, int W, int kd, void* stream);

/* Weight gradient of the same stride-1 convolutions in Winograd form: gw = G^T [ sum_tiles (A gy A^T) (.) (B^T x B) ] G, the
 * per-lane operand transforms done on the fly from the raw LDS tiles of ecm_conv3d_k3_wgrad's kernel (conv3d_wgrad.hip).
 * kd = 3: x [B,Ci,D,H,W], gy [B,Co,D,H,W] -> gw [Co,Ci,3,3,3];  kd = 1 (D independent planes): gw [Co,Ci,3,3].  Deterministic. */
long long ecm_conv_wino_wgrad_scratch_bytes(int B, int Ci, int Co, int D, int H, int W, int kd);
int ecm_conv_wino_wgrad(const float* x, const float* gy, float* gw, void* scratch, long long scratch_bytes, int B, int Ci,
                        int Co, int D, int H, int W, int kd, void* stream);

/* The classifier's last layer Conv3d(Ci<=32 -> 1) (cmfsm.py:624,629,634) on its own kernels: w is the reference weight
 * [1,Ci,3,3,3] (no packing); y: [B,1,D,H,W].  wgrad: gw [1,Ci,27] from x [B,Ci,D,H,W] and gy [B,1,D,H,W]. */
int ecm_conv3d_c1_fwd(const float* x, const float* w, float* y, int B, int Ci, int D, int H, int W, void* stream);
/* data gradient of the same layer: gx[B,Ci,D,H,W] from gy[B,1,D,H,W] and w[1,Ci,27] (any Ci). */
int ecm_conv3d_c1_dgrad(const float* gy, const float* w, float* gx, int B, int Ci, int D, int H, int W, void* stream);
long long ecm_conv3d_c1_wgrad_scratch_bytes(int B, int Ci, int D, int H, int W);
int ecm_conv3d_c1_wgrad(const float* x, const float* gy, float* gw, void* scratch, long long scratch_bytes,
                        int B, int Ci, int D, int H, int W, void* stream);
/* ABI 4: the whole tail of a classifier, GroupNorm(32) + ReLU + Conv3d(32 -> 1) (cmfsm.py:621-634: classifN[0][1], [1], [2]),
 * with the normalisation applied while x is staged: x is the RAW output of classifN[0][0] and mean_rstd [B,32,2] its group
 * statistics from ecm_gn3d_stats; h = relu(gn(x)) is never written.  Ci must be 32 (one channel per group; any other positive Ci:
 * ECM_EUNSUP).  fwd: y [B,1,D,H,W];
 * wgrad: gw [1,32,27] = sum gy (x) h.  The data gradient w.r.t. h is ecm_conv3d_c1_dgrad, the GroupNorm backward
 * ecm_gn3d_bwd with y == NULL (ReLU mask recomputed from x). */
int ecm_conv3d_c1_gn_fwd(const float* x, const float* mean_rstd, const float* gamma, const float* beta, const float* w,
                         float* y, int B, int Ci, int D, int H, int W, void* stream);
int ecm_conv3d_c1_gn_wgrad(const float* x, const float* mean_rstd, const float* gamma, const float* beta, const float* gy,
                           float* gw, void* scratch, long long scratch_bytes, int B, int Ci, int D, int H, int W, void* stream);

/* ConvTranspose3d k=3, stride 2, pad 1, output_padding 1 (cmfsm.py:262-281): x [B,Ci,D,H,W] -> y [B,Co,Do,Ho,Wo],
 * Do = 2D (or 2D-1 when used as the data gradient of a stride-2 conv over an odd extent).
 * Weight in the reference layout [Ci,Co,3,3,3]; a Conv3d weight [Co_f,Ci_f,27] is the same memory layout
 * for its own data gradient (Ci := Co_f, Co := Ci_f).  packed: 27*Ci*CoP floats.  Ci % 4 == 0 and Co <= 64, and every output
 * extent 2n or 2n-1, else ECM_EUNSUP; a zero or negative Ci, Co or extent: ECM_EINVAL.  So for the 2-D deconvolutions below. */
int ecm_deconv3d_pack_weight(const float* w, float* packed, int Ci, int Co, void* stream);
int ecm_deconv3d_k3s2_fwd(const float* x, const float* wpacked, float* y,
                          int B, int Ci, int Co, int D, int H, int W, int Do, int Ho, int Wo, void* stream);

/* gw[co,ci,27] (reference Conv3d layout) = sum_{b,o} gy[b,co,o] * x[b,ci,o*st+k-1].
 * x: [B,Ci,D,H,W], gy: [B,Co,Do,Ho,Wo]; scratch >= ecm_conv3d_wgrad_scratch_bytes(...) */
long long ecm_conv3d_wgrad_scratch_bytes(int B, int Ci, int Co, int D, int H, int W, int stride);
int ecm_conv3d_k3_wgrad(const float* x, const float* gy, float* gw, void* scratch, long long scratch_bytes,
                        int B, int Ci, int Co, int D, int H, int W, int stride, void* stream);

/* General 2-D convolution family (conv2d.hip), same implicit-GEMM kernel: the encoder's Conv2d layers (feature_extraction,
 * cmfsm.py:126-236: 3x3 with stride 1|2 and dilation 1|2|4, the 3-channel stem, 64/128/320-channel stages, 1x1 projections),
 * the class-indexed convolutions of the collapsed cost volume (3x3 32->480, sheared 3x5 32->192; cmfsm.py:667-684) and all
 * stride-1 data gradients (flip_transpose packing).  (kh,kw,stride,dil) in {(3,3,1,1|2|4), (3,3,2,1), (3,5,1,1), (1,1,1|2,1)}.
 *   y[b,co,oh,ow] = sum w[co,ci,i,j] x[b,ci,oh*stride - pad_top + i*dil, ow*stride - pad_left + j*dil]   (0 outside x)
 * x: [B,Ci,H,W]; y: [B,Co,Ho,Wo] -- Ho, Wo and the top/left padding are given explicitly (the bottom/right padding is
 * whatever Ho, Wo imply), which also covers asymmetric padding.  packed: ecm_conv2d_packed_floats_ex floats, filled by
 * ecm_conv2d_pack_weight_ex from the reference layout [Co,Ci,kh,kw] (flip_transpose: the data-gradient operator with
 * Cin' = Co, Cout' = Ci; call the size query with the swapped channel counts). */
long long ecm_conv2d_packed_floats_ex(int Ci, int Co, int kh, int kw);
int ecm_conv2d_pack_weight_ex(const float* w, float* packed, int Co, int Ci, int kh, int kw, int flip_transpose, void* stream);
int ecm_conv2d_fwd_ex(const float* x, const float* wpacked, float* y, int B, int Ci, int Co, int H, int W, int kh, int kw,
                      int stride, int dil, int pad_top, int pad_left, int Ho, int Wo, void* stream);
/* gw[co,ci,kh,kw] = sum_{b,oh,ow} gy[b,co,oh,ow] x[b,ci,oh*stride - pad_top + i*dil, ow*stride - pad_left + j*dil] for the
 * same family; gy: [B,Co,Ho,Wo].  Deterministic (per-workgroup partials, fixed-order sum).  The size
 * query also answers outside the family (with the caller's kh * kw taps): there a short scratch is ECM_ESCRATCH and, with room,
 * the call ECM_EUNSUP. */
long long ecm_conv2d_wgrad_ex_scratch_bytes(int B, int Ci, int Co, int Ho, int Wo, int kh, int kw, int stride);
int ecm_conv2d_wgrad_ex(const float* x, const float* gy, float* gw, void* scratch, long long scratch_bytes, int B, int Ci,
                        int Co, int H, int W, int kh, int kw, int stride, int dil, int pad_top, int pad_left, int Ho, int Wo,
                        void* stream);
/* Data gradient of a stride-2 3x3 Conv2d (pad 1) = ConvTranspose2d(k 3, stride 2, pad 1): x [B,Ci,H,W] -> y [B,Co,Ho,Wo],
 * Ho in {2H-1, 2H}.  w: a Conv2d weight [Co_f = Ci here, Ci_f = Co here, 3, 3] as it stands.  Co <= 64, Ci % 4 == 0. */
int ecm_deconv2d_pack_weight(const float* w, float* packed, int Ci, int Co, void* stream);
int ecm_deconv2d_k3s2_fwd(const float* x, const float* wpacked, float* y, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                          void* stream);

/* ---- cmf decoder, super_resolution_refinement (cmf.py:227-264) ----------------------------------------------------------
 * ConvTranspose2d(Ci, Co, 3, stride 2, pad 1, output_padding 1, bias=True) (deconv_module_list.i.0, cmf.py:236-239): the
 * kernel of ecm_deconv2d_k3s2_fwd with bias[co] added in its epilogue.  w: the ConvTranspose2d weight [Ci,Co,3,3], packed by
 * ecm_deconv2d_pack_weight(w, packed, Ci, Co); bias [Co].  Co <= 64, Ci % 4 == 0, Ho in {2H-1, 2H}. */
int ecm_deconv2d_k3s2_bias_fwd(const float* x, const float* wpacked, const float* bias, float* y, int B, int Ci, int Co, int H,
                               int W, int Ho, int Wo, void* stream);
/* out[c] = sum_{b,p} x[b,c,p] over x [B,C,HW]: the bias gradient of a layer whose output gradient is x.  Fixed-order partial
 * sums (no atomics): bit-reproducible.  scratch >= ecm_channel_sum_scratch_bytes(B, C, HW). */
long long ecm_channel_sum_scratch_bytes(int B, int C, long long HW);
int ecm_channel_sum(const float* x, float* out, void* scratch, long long scratch_bytes, int B, int C, long long HW, void* stream);
/* conv_out + crap (cmf.py:259-264): y = relu(Conv2d(Ci -> 1, 3x3, pad 1, bias)(x)), x [B,Ci,H,W] -> y [B,1,H,W].
 * w: the reference weight [1,Ci,3,3] as it stands (no packing), bias [1].
 * dgrad: gx [B,Ci,H,W] from gy [B,1,H,W] masked by the forward output y (> 0).
 * wgrad: gw [1,Ci,3,3] and gb [1] from x, gy and y; fixed-order reductions, bit-reproducible;
 *        scratch >= ecm_conv2d_c1_wgrad_scratch_bytes(...). */
int ecm_conv2d_c1_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, void* stream);
int ecm_conv2d_c1_dgrad(const float* gy, const float* y, const float* w, float* gx, int B, int Ci, int H, int W, void* stream);
long long ecm_conv2d_c1_wgrad_scratch_bytes(int B, int Ci, int H, int W);
int ecm_conv2d_c1_wgrad(const float* x, const float* gy, const float* y, float* gw, float* gb, void* scratch,
                        long long scratch_bytes, int B, int Ci, int H, int W, void* stream);

/* GroupNorm(32 groups, eps) over [B,C,S] (S = D*H*W), cmfsm.py:58; deterministic fixed-order reductions.
 * scratch for every call: >= ecm_gn3d_scratch_bytes(B,C,S) (0 for sizes the entries refuse: C % 32 != 0 is ECM_EUNSUP).
 * fwd: y = relu?( (x-mean)*rstd*gamma[c]+beta[c] (+ skip) ) (skip may be NULL) and mean_rstd [B,32,2] in ONE pass over x
 *      (a cluster of co-resident workgroups keeps the span in registers across the reduction); shapes that do not fit
 *      that kernel run the two-stage forward below. */
long long ecm_gn3d_scratch_bytes(int B, int C, long long S);
int ecm_gn3d_fwd(const float* x, const float* gamma, const float* beta, const float* skip, float* y,
                 float* mean_rstd, void* scratch, long long scratch_bytes, int B, int C, long long S,
                 int relu, float eps, void* stream);
/* The two-stage forward, also the storage conversions of the bf16 inference paths (ops.aggregation_dtype / encoder_dtype).
 * bf16 travels as its bit pattern (unsigned short); every bf16 output is rounded once (round to nearest even, NaN stays NaN).
 * stats: mean_rstd [B,32,2] fp32 of an fp32 or (_bf16) a bf16 x, one variance formulation for both; scratch >=
 * ecm_gn3d_scratch_bytes(B,C,S).  apply: y = relu?( GroupNorm(x)*gamma + beta (+ skip) ), skip NULL or of x's shape, from
 * mean_rstd of the matching stats call:
 *   ecm_gn3d_apply           fp32 x, fp32 skip -> fp32 y
 *   ecm_gn3d_apply_bf16      bf16 x, bf16 skip -> bf16 y
 *   ecm_gn3d_apply_f32_bf16  fp32 x, bf16 skip -> bf16 y   (the boundary into the bf16 aggregation region)
 *   ecm_gn3d_apply_bf16_f32  bf16 x, bf16 skip -> fp32 y32 and, with y16 non-NULL, the same values rounded to bf16 (the
 *                            encoder's results; y16 for those that also feed its next layer) */
int ecm_gn3d_stats(const float* x, float* mean_rstd, void* scratch, long long scratch_bytes,
                   int B, int C, long long S, float eps, void* stream);
int ecm_gn3d_stats_bf16(const unsigned short* x, float* mean_rstd, void* scratch, long long scratch_bytes,
                        int B, int C, long long S, float eps, void* stream);
int ecm_gn3d_apply(const float* x, const float* mean_rstd, const float* gamma, const float* beta,
                   const float* skip, float* y, int B, int C, long long S, int relu, void* stream);
int ecm_gn3d_apply_bf16(const unsigned short* x, const float* mean_rstd, const float* gamma, const float* beta,
                        const unsigned short* skip, unsigned short* y, int B, int C, long long S, int relu, void* stream);
int ecm_gn3d_apply_f32_bf16(const float* x, const float* mean_rstd, const float* gamma, const float* beta,
                            const unsigned short* skip, unsigned short* y, int B, int C, long long S, int relu, void* stream);
int ecm_gn3d_apply_bf16_f32(const unsigned short* x, const float* mean_rstd, const float* gamma, const float* beta,
                            const unsigned short* skip, float* y32, unsigned short* y16, int B, int C, long long S, int relu,
                            void* stream);
/* The one-pass forms of ecm_gn3d_fwd / ecm_gn3d_bwd make workgroups of one launch wait for each other (a cluster of
 * <= 128 workgroups per (sample, group) span exchanges partial sums).  Members are assigned by tickets drawn at run
 * time, so progress needs only one cluster's worth of this launch's workgroups running, whatever else shares the
 * device; every wait is bounded in wall time.  If a bound expires (device shared so heavily that a cluster never became
 * resident within the poll time), the affected outputs are NaN AND a sticky, process-wide error word is set from the
 * device: every later ecm_gn3d_* call returns ECM_EASYNC, and ecm_async_status(clear) reports (and optionally clears) it
 * -- call it after synchronising the stream at the end of a step.  Never a hang, never a silent success.
 *   ecm_gn3d_cluster_mode(mode): 1 = cluster kernels (default), 0 = two-stage kernels only (no inter-workgroup waits:
 *     the safe choice when many processes share one device), 2 / 3 = diagnostics (static member ids / undersized grid that
 *     forces the timeout path), 4 = as 1, and ALSO on a stream that is being captured into a HIP graph (by default a capturing
 *     stream gets the two-stage kernels: two graphs with cluster launches replayed concurrently would starve each other, and
 *     cluster launches of one process are otherwise ordered across streams by the library -- mode 4 is the caller's promise
 *     that such graphs replay one at a time); any other value only queries.  Returns the previous mode.  Env
 *     ECM_GN_CLUSTER_MODE presets it.
 *   ecm_gn3d_poll_ms(ms): wait bound in milliseconds (default 2000; ms <= 0 only queries).  Returns the previous bound.  Env
 *     ECM_GN_POLL_MS presets it.
 *   Both read their environment preset at the first call of either, or at the first GroupNorm launch, whichever comes first:
 *   a query as the very first call reports the preset, and a value set by a call is never replaced by the preset later. */
int ecm_gn3d_cluster_mode(int mode);
int ecm_gn3d_poll_ms(int ms);
int ecm_async_status(int clear);

/* Backward of y = relu?(gn(x) + skip): writes gx, gskip (NULL to skip it), ggamma[C] and gbeta[C].
 * ReLU mask (relu != 0): from the forward OUTPUT y when y != NULL; with y == NULL it is recomputed from x, which needs
 * beta and is only valid for a forward WITHOUT skip (saves one tensor read per pass).  beta may be NULL otherwise. */
int ecm_gn3d_bwd(const float* x, const float* mean_rstd, const float* gamma, const float* beta, const float* y,
                 const float* gy, float* gx, float* gskip, float* ggamma, float* gbeta, void* scratch,
                 long long scratch_bytes, int B, int C, long long S, int relu, void* stream);

/* The class-indexed 2-D kernels of that collapse from dres0[0][0].weight w [Co,2C,3,3,3] (reference layout):
 * wP [15,Co,C,3,3] (one 3x3 kernel per (wedge class, depth-edge class) of the reference-image half) and wQ [6,Co,C,3,5]
 * (sheared 3x5 kernels of the target-image half); bwd: gw from (gwP, gwQ), every element written. */
int ecm_costvol_class_weights_fwd(const float* w, float* wP, float* wQ, int Co, int C, void* stream);
int ecm_costvol_class_weights_bwd(const float* gwP, const float* gwQ, float* gw, int Co, int C, void* stream);

/* The same two calls for a caller that KEEPS the one-pass kernels' exchange memory across calls: `cluster` is a device
 * buffer of >= ecm_gn3d_cluster_bytes(B) bytes that was filled once by ecm_gn3d_cluster_preset (all-ones) and is used by one
 * stream at a time.  The kernels leave it in the preset state when they finish (the last member of a cluster restores the
 * cluster's slots, the last ticket draw the ticket counter), so no memset is issued per launch (ecm_gn3d_fwd / _bwd issue one:
 * 172 per cmfsm training step).  After an asynchronous time-out (ECM_EASYNC) the buffer must be preset again.  `scratch` as
 * for ecm_gn3d_fwd / _bwd (two-stage partials and the per-channel sums).
 * The one-pass kernels keep 64 KB of dynamic LDS per workgroup (two workgroups per CU): part of a slab's output waits there and
 * is stored under the NEXT slab's exchange (csrc/gn3d.hip: STASH_V4).  y / gx must not alias any input of the call. */
long long ecm_gn3d_cluster_bytes(int B);
int ecm_gn3d_cluster_preset(void* cluster, long long cluster_bytes, void* stream);
int ecm_gn3d_fwd_p(const float* x, const float* gamma, const float* beta, const float* skip, float* y,
                   float* mean_rstd, void* scratch, long long scratch_bytes, void* cluster, long long cluster_bytes,
                   int B, int C, long long S, int relu, float eps, void* stream);
int ecm_gn3d_bwd_p(const float* x, const float* mean_rstd, const float* gamma, const float* beta, const float* y,
                   const float* gy, float* gx, float* gskip, float* ggamma, float* gbeta, void* scratch,
                   long long scratch_bytes, void* cluster, long long cluster_bytes, int B, int C, long long S,
                   int relu, void* stream);

/* Cost volume + dres0's first Conv3d (cmfsm.py:667-684) without the 4-D volume: both halves of the concat volume are
 * constant along a line in (d,x), so the 3x3x3 convolution collapses to 2-D convolutions of the feature maps (host side):
 *   P[b, classP, co, y, x]     classP(d,x) = (clamp(d-x,-2,2)+2)*3 + edge(d)        15 classes, reference-image half
 *   Qp[b, classQ, co, y, u+2]  classQ(d,x) = edge(d)*2 + (x == w-1), u = x-d         6 classes, target-image half (3x5)
 *   edge(d) = 0 / 1 / 2 for d == 0 / interior / d == D-1
 * fwd: y[B,Co,D,h,w] = P[classP(d,x)][x] + Qp[classQ(d,x)][x-d+2] where d-x < 3, else 0.
 * bwd: gP [B,15,Co,h,w], gQp [B,6,Co,h,w+2] = sums of gy over the d of each class (adjoint of fwd).  D >= 2 (D = 1: ECM_EUNSUP;
 * D <= 0: ECM_EINVAL). */
int ecm_costvol_conv_assemble_fwd(const float* P, const float* Qp, float* y, int B, int Co, int D, int h, int w, void* stream);
int ecm_costvol_conv_assemble_bwd(const float* gy, float* gP, float* gQp, int B, int Co, int D, int h, int w, void* stream);

/* Input side of the harness (cmf/loader/Flying3d.py:49-99): a batch of resident float32 frames [B,H,W,7] = (left RGB,
 * right RGB, disparity) -> left, right [B,3,th,tw] = ((v/255) - mean[c]) / std[c], disp [B,th,tw], and optionally
 * image [B,3,th,tw] = the raw left image in CHW (NULL to skip).  Output row r < split reads frame row crop_y0[b]+r, row
 * r >= split reads frame row H-tail+(r-split) (eval: split 540, tail 36 -> 576 rows; train: split == th); columns
 * crop_x0[b] .. +tw.  crop_y0 / crop_x0 / mean3 / std3 are HOST arrays (B ints / 3 floats).  Bit-identical to the loader. */
int ecm_frame_prep(const float* frames, float* left, float* right, float* disp, float* image, int B, int H, int W,
                   const int* crop_y0, const int* crop_x0, int th, int tw, int split, int tail,
                   const float* mean3, const float* std3, void* stream);

/* KITTI evaluation frames (cmf/loader/KITTI.py:98-108): pad [B,H,W,7] frames to th x tw (384 x 1248) at the TOP and LEFT
 * by repeating the first th-H rows / tw-W columns; disparity is 0 wherever the source row < th-H or the source column <
 * tw-W (the loader zeroes it through numpy views, which also hits the un-padded frame).  Needs th-H <= H, tw-W <= W. */
int ecm_frame_prep_kitti_eval(const float* frames, float* left, float* right, float* disp, float* image, int B,
                              int H, int W, int th, int tw, const float* mean3, const float* std3, void* stream);

/* Packed shards (frame contents per flying3ddata.py:34-39): rgb6 uint8 [B,H,W,6] (left RGB, right RGB) and
 * disp_in [B,H,W] as fp16 (disp_is_half != 0) or fp32.  Same outputs and arithmetic as ecm_frame_prep; mode 0 = the
 * window / split-tail form with crop_y0/crop_x0/split/tail as there, mode 1 = the KITTI top-left padding (crop arrays,
 * split and tail ignored).  Colour outputs are bit-identical to the float32-frame path on the same pixel values. */
int ecm_frame_prep_packed(const unsigned char* rgb6, const void* disp_in, int disp_is_half, float* left, float* right,
                          float* disp, float* image, int B, int H, int W, const int* crop_y0, const int* crop_x0,
                          int th, int tw, int split, int tail, const float* mean3, const float* std3, int mode, void* stream);

/* SceneFlow evaluation (test.py:69-94): pred [B,Hp,Wp] (= output3 squeezed) and gt [B,Hg,Wg], both cropped to
 * [:crop_h, :crop_w] (540 x 960).  out6 (device) = [epe, epe_non, epe_true, n, n_non, n_true]: mean |pred - gt| under
 *   mask = 0 <= gt < maxdisp;  mask_non = mask and x - gt >= 0;  mask_true = 0 < gt < maxdisp and x - gt >= 0
 * (x = column index).  An empty mask gives NaN like the reference's mean of an empty selection. */
long long ecm_eval_epe_scratch_bytes(long long n);
int ecm_eval_epe(const float* pred, const float* gt, float* out6, void* scratch, long long scratch_bytes, int B,
                 int Hp, int Wp, int Hg, int Wg, int crop_h, int crop_w, float maxdisp, void* stream);

/* KITTI validation (eval_kitti.py:84-103): pred [B,H,W] (= output3 squeezed) against gt [B,H,W] on the whole frame, no crop;
 * x = column index as a float, every comparison and |pred - gt| in fp32:
 *   mask = 0 < gt < maxdisp;   mask_non = mask_true = mask and x - gt >= 0   (the reference writes these two identically:
 *   both columns are kept so that a caller's log has the reference's names, and they always hold the same values);
 *   good = |pred - gt| < 3 or |pred - gt| < 0.05f * gt, under mask.
 * out8 (device) = [loss, loss_non, loss_true, loss_3, n_mask, n_non, n_true, n_good]: the three masked means of |pred - gt|
 * (fp32 partial sums, final sum in double), loss_3 = 100 - n_good / n_mask * 100 in fp32 as the reference forms it, and the
 * counts, accumulated as integers and written as floats.  An empty mask gives NaN for its mean and for loss_3, like the
 * reference's mean of an empty selection and its 0 / 0.  A NaN prediction under the mask makes the means NaN and is not good.
 * per_sample (device, [B,8], may be NULL) = the same eight columns of each image alone -- an addition: the reference has
 * only the batch row.  Uses 16-byte loads when W % 4 == 0 and pred, gt are 16-byte aligned; any 4-byte alignment works.
 * No atomics: bit-reproducible.  B, H, W >= 1, else ECM_EINVAL; H * W >= 2^31 or B > 65535: ECM_EUNSUP. */
long long ecm_eval_kitti_scratch_bytes(int B, int H, int W);
int ecm_eval_kitti(const float* pred, const float* gt, float* out8, float* per_sample, void* scratch, long long scratch_bytes,
                   int B, int H, int W, float maxdisp, void* stream);

/* ABI 15: sparsification curves of K confidence planes and of the oracle, per sample.  Nothing in the
 * reference corresponds to it.  pred, gt [B,H,W] fp32; measures: a HOST array of K device pointers, each a [B,H,W] fp32 plane in
 * which a HIGHER value means LESS trusted.  Per sample:
 *   valid    0 < gt < maxdisp; n valid pixels.
 *   error    e = |pred - gt| in fp32, entering every sum as the integer E = rintf(min(e, 4095) * 65536) (a NaN e takes the clamp;
 *            E < 2^28, the scaling is exact, a mean moves by at most 2^-17 px); bad = not (e < 3 or e < 0.05f * gt).
 *   key      of a measure value: its order-preserving 32-bit image (all bits flipped if the sign bit is set, else the sign bit
 *            set), -0.0 taken as +0.0, any NaN 0xFFFFFFFF (removed first).  Plane K, the oracle, has the key E.
 *   cuts     r_j = floor(j * n / steps), j = 0..steps-1.  With the valid pixels grouped by equal key and ranked from the highest
 *            key down, A = the groups strictly above the group (c, E_t, bad_t) that holds rank r_j, t = r_j - n_A; in fp64, in
 *            this order:  remE = (E_tot - E_A) - t * E_t / c;  rembad = (bad_tot - bad_A) - t * bad_t / c  (ties leave pro rata);
 *            epe_j = (float)(remE / (n - r_j) / 65536);  d1_j = (float)(100 * rembad / (n - r_j)).
 * table (device) fp32 [B, K+1, steps, 2] = (epe_j, d1_j); plane K is the oracle, whose d1 column holds the closed form
 * (float)(100 * (bad_tot - min(r_j, bad_tot)) / (n - r_j)).  count (device) int64 [B,3] = (n, E_tot, bad_tot).  n = 0: NaN rows.
 * Exact on the full 32-bit key (a radix selection, four digits of 8 bits; nothing is sorted).  Integer accumulation only (integer
 * atomics commute): bit-reproducible, and row b does not depend on the other samples.  16-byte loads when W % 4 == 0 and pred,
 * gt and every plane are 16-byte aligned; any 4-byte alignment works.  scratch: 8-byte aligned, ecm_eval_sparsify_scratch_bytes
 * (0 for sizes outside the limits); too small: ECM_ESCRATCH and nothing is launched.  B, H, W, K, steps >= 1, else ECM_EINVAL;
 * H * W >= 2^31, B > 65535, K > ecm_eval_sparsify_max_measures() (8) or steps > ecm_eval_sparsify_max_steps() (64): ECM_EUNSUP.
 * The three queries need no GPU. */
int ecm_eval_sparsify_max_measures(void);
int ecm_eval_sparsify_max_steps(void);
long long ecm_eval_sparsify_scratch_bytes(int B, int H, int W, int K, int steps);
int ecm_eval_sparsify(const float* pred, const float* gt, const float* const* measures, float* table, long long* count,
                      void* scratch, long long scratch_bytes, int B, int H, int W, int K, int steps, float maxdisp, void* stream);

/* KITTI submission image (test_kitti.py:163-168): out[b,y,x] = (uint16)(pred[b, Hp-h[b]+y, Wp-w[b]+x] * scale) for
 * y < h[b], x < w[b] (the loader padded at the top and left), 0 elsewhere; scale = 256.  The cast is numpy's on the
 * reference's host: truncation toward zero, low 16 bits of the 32-bit integer, 0 for NaN / out-of-int32-range values.
 * pred: [B,Hp,Wp]; out: uint16 [B,Ho,Wo]; h, w: HOST arrays of B ints.  Integer output: bit-exact. */
int ecm_disp_to_u16(const float* pred, unsigned short* out, int B, int Hp, int Wp, const int* h, const int* w,
                    int Ho, int Wo, float scale, void* stream);

/* ABI 10: left-right consistency check of two disparity maps in one kernel (the cross-check that users of
 * the reference run in numpy on the host).  dl [B,H,W]: left-view disparity in pixels; dr [B,H,W]: right-view disparity in
 * right-image coordinates (right pixel x' matches left pixel x' + dr); with mirrored != 0 dr is stored flipped along W (element
 * x' at W-1-x': what a forward pass on the two flipped images returns).  Per pixel, d = dl[b,y,x], all in fp32:
 *   xr = x - d;  x0 = floor(xr);  x1 = min(x0 + 1, W-1);  t = xr - x0;  r = dr[x0] + t (dr[x1] - dr[x0]) on the same row;
 *   tol = max(threshold, rel * d);  error = |d - r|, +inf where kind is 3 or r is not finite;
 *   kind = 3 (out of view) if d is not finite or xr < 0 or xr > W-1;  else 0 (consistent) if error <= tol;  else 1 (occluded)
 *          if r is finite and r > d;  else 2 (mismatch);
 *   filled = d where kind is 0, else dl at the nearest consistent column of the row on the left or on the right, whichever holds
 *          the smaller disparity (the left one on a tie; the only one if the other side has none), 0 if the row has none.
 * check: [3,B,H,W] = (error, kind, filled), kind a float plane of exact integers.  src (int [B,H,W], may be NULL): the column
 * `filled` was copied from, -1 for none.  One launch, a workgroup per row at a time; no atomics: bit-reproducible.
 * threshold, rel >= 0 and finite, B, H, W >= 1, else ECM_EINVAL; W > ecm_lr_check_max_width() or B * H >= 2^31: ECM_EUNSUP,
 * before any launch. */
int ecm_lr_check_max_width(void);
int ecm_lr_check_fwd(const float* dl, const float* dr, float* check, int* src, int B, int H, int W, float threshold, float rel,
                     int mirrored, void* stream);

/* ABI 11: image-space post-filters of a disparity map (the median and the guided bilateral filter that end
 * the classical stereo pipeline and that users of the reference run with OpenCV or numpy on the host).  All arithmetic in fp32.
 *   Usable sample.  d [B,H,W] fp32, valid [B,H,W] unsigned char (NULL: all ones).  A sample q is usable iff it lies inside the
 *     image, d[q] is finite and valid[q] != 0.  Windows are clipped to the image: a position outside it is excluded exactly like
 *     an invalid one; no padding, no replication.
 *   Masked median, radius r in 1..ecm_disp_filter_max_radius(ECM_DISP_FILTER_MEDIAN) = 3 (3x3, 5x5, 7x7).  m = the number of
 *     usable samples in the (2r+1)^2 window about p (the centre counts if it is usable); median[p] = the LOWER median, the value
 *     of rank floor((m-1)/2), 0-based and ascending, among them -- one of the inputs, bit for bit (+0 and -0 compare equal) -- and
 *     0, KITTI's invalid value, where m == 0; support[p] = m, a float plane of exact integers.  out [2,B,H,W] = (median, support).
 *   Joint bilateral, radius r in 1..ecm_disp_filter_max_radius(ECM_DISP_FILTER_BILATERAL) = 8 (17x17), guide g [B,C,H,W] fp32,
 *     C in 1..4.  For a usable q = p + (dx, dy) of the clipped window
 *       w(q) = exp( -(dx^2 + dy^2) / (2 sigma_space^2) - sum_c (g_c[p] - g_c[q])^2 / (2 sigma_color^2) );
 *     a sample whose exponent is NaN (a non-finite guide value at p or at q) is excluded.  refined[p] = sum w d / sum w where
 *     sum w > 0, else 0; weight[p] = sum w.  The centre is included when it is usable (w = 1); a pixel whose centre is not usable
 *     is written all the same, from its neighbours: the hole filling.  out [2,B,H,W] = (refined, weight).
 * One launch each, LDS-tiled, no scratch, no atomics: bit-reproducible.  Neither H nor W has an upper bound; B * H * W >= 2^31
 * returns ECM_EUNSUP before any launch.  ECM_EINVAL, before any device work: a null d / guide / out, B, H or W < 1, a radius out
 * of range, C outside 1..4, a sigma that is not finite and positive.  ecm_disp_filter_max_radius is a size query (no GPU);
 * ECM_EINVAL for an unknown kind. */
#define ECM_DISP_FILTER_MEDIAN    0
#define ECM_DISP_FILTER_BILATERAL 1
int ecm_disp_filter_max_radius(int kind);
int ecm_disp_median_fwd(const float* d, const unsigned char* valid, float* out, int B, int H, int W, int radius, void* stream);
int ecm_disp_bilateral_fwd(const float* d, const unsigned char* valid, const float* guide, float* out, int B, int C, int H, int W,
                           int radius, float sigma_space, float sigma_color, void* stream);

/* ABI 12: the speckle filter of a disparity map (OpenCV's filterSpeckles, which users of the reference run on
 * the host): the connected segments of near-constant disparity, and the map with the small ones removed.
 *   Usable.  As in ABI 11: d [B,H,W] fp32, valid [B,H,W] unsigned char (NULL: all ones); a pixel is usable iff d is finite and
 *     valid != 0.
 *   Connected.  Two usable pixels of the same image are connected iff they are 4-neighbours (left/right/up/down: no diagonals, no
 *     wrap from the end of a row to the start of the next or from one image to the next) and |d[p] - d[q]| <= max_diff, evaluated
 *     in fp32 and inclusive.
 *   Segment.  A connected component of that graph.  The relation is not transitive: a ramp whose step is <= max_diff is one
 *     segment although its ends differ by much more.
 *   segments [2,B,H,W] int32 = (label, size): label[p] = the row-major index y*W + x, within its image, of the first pixel of p's
 *     segment, -1 where p is not usable; size[p] = the segment's pixel count, 0 where p is not usable.
 *   out [B,H,W] fp32: d[p], bit for bit, where p is usable and size[p] > max_size; 0 elsewhere.  A segment is removed iff its size
 *     is <= max_size (filterSpeckles' rule); with max_size = 0 nothing usable is removed.  out must not overlap d.
 * Four launches on `stream` (union-find over int32 parents: per tile in LDS, across tile borders by agent-scope atomic min, then a
 * count and a broadcast); `segments` and `out` double as the working arrays, so there is no scratch buffer.  Integer atomics only,
 * and label is a minimum and size a sum of integers: bit-reproducible.  No kernel waits for another workgroup.  Neither H nor W has
 * an upper bound; B * H * W >= 2^31 returns ECM_EUNSUP before any launch.  ECM_EINVAL, before any device work: a null d, out or
 * segments, B, H or W < 1, max_size < 0, max_diff negative or not finite. */
int ecm_disp_speckle_fwd(const float* d, const unsigned char* valid, float* out, int* segments, int B, int H, int W, int max_size,
                         float max_diff, void* stream);

/* ABI 13: the WLS disparity smoother: the confidence-weighted, edge-aware global smoother that ends OpenCV's
 * post-processing chain (DisparityWLSFilter; the fast global smoother of Min et al. 2014).  All device arithmetic in fp32.
 *   Inputs.  d [B,H,W] fp32 (pixels), guide g [B,C,H,W] fp32 with C in 1..4, conf [B,H,W] fp32 (NULL: all ones).
 *   Usable pixel.  d[p] finite, conf[p] finite and conf[p] >= 0; where a pixel is not usable both its d and its conf count as 0.
 *   Link weights.  Between horizontal neighbours p = (y,x), q = (y,x+1): w = exp(-sqrt(sum_c (g_c[p] - g_c[q])^2) / sigma_color),
 *     the vertical ones alike; a weight that is NaN (a non-finite guide value) is 0: the link is cut.
 *   One line solve, length n, right-hand side f, weights w_0..w_{n-2}, strength L: (I + L A) u = f with a_i = -L w_{i-1} (a_0 = 0),
 *     c_i = -L w_i (c_{n-1} = 0), b_i = 1 - a_i - c_i, by the Thomas algorithm in natural order: den = b_i - a_i c'_{i-1},
 *     c'_i = c_i / den, f'_i = (f_i - a_i f'_{i-1}) / den, then u_i = f'_i - c'_i u_{i+1}.  Strictly diagonally dominant: no pivoting.
 *   Schedule.  N = conf * d, D = conf; for t = 1..T with L_t = 1.5 * 4^(T-t) / (4^T - 1) * lam (formed in double from the fp32 lam,
 *     then rounded to fp32): every row of N and of D with the horizontal weights, then every column with the vertical ones.  N and
 *     D go through the same instructions with the same coefficients.
 *   out [2,B,H,W] = (smoothed, weight): smoothed = N / D (a true IEEE division) where D > 0, else 0; weight = D.  A constant
 *     power-of-two plane comes back bit for bit wherever D > 0; a region that cut links separate from every confident pixel has
 *     D == 0 exactly and is 0.
 * 2T launches on `stream` (a row pass and a column pass per iteration; forward and backward sweep of a pass in one kernel, one
 * lane per line).  `out` holds N and D between the passes; scratch (ecm_disp_wls_scratch_bytes(B, H, W) bytes, a size query that
 * needs no GPU: the c' plane) is written before it is read.  out and scratch must not overlap d, conf or guide.  No atomics, no
 * workgroup waits for another: bit-reproducible.  Neither H nor W has an upper bound; B * H * W >= 2^31 returns ECM_EUNSUP before
 * any launch.  ECM_EINVAL, before any device work: a null d / guide / out / scratch, B, H or W < 1, C outside 1..4, lam or
 * sigma_color not finite and positive, iterations outside 1..8 (the size query: B, H or W < 1). */
long long ecm_disp_wls_scratch_bytes(int B, int H, int W);
int ecm_disp_wls_fwd(const float* d, const float* conf, const float* guide, float* out, void* scratch, int B, int C, int H, int W,
                     float lam, float sigma_color, int iterations, void* stream);

/* ABI 14: the forward warp ("splat") of a left disparity map into the right view: the right view's
 * disparity, and with it the occlusions, from ONE inference instead of two.  dl [B,H,W] fp32: left-view disparity in pixels.
 *   Candidate.  Pixel x of a row, d = dl[b,y,x], is a candidate iff d is finite and xr = (float)x - d, one fp32 subtraction, lies
 *     in [0, W-1]: the in-view rule of ABI 10.  With f = floorf(xr) it lands on column x0 = (int)f and, if xr > f, also on
 *     x1 = min(x0 + 1, W-1): exactly the one or two columns ecm_lr_check_fwd reads for that pixel.
 *   Key.  A 64-bit unsigned word: the high 32 bits the order-preserving image of d's bits (every bit flipped if the sign bit is
 *     set, else the sign bit set; unsigned order is then float order with -0.0 < +0.0), the low 32 bits the source column x.
 *     Every finite float's image is >= 0x00800000, so the word 0 means that nothing landed.
 *   Winner.  Per right-view column the candidate with the largest key: the largest disparity (the nearest surface), and among
 *     equal disparities the larger source column.
 *   right [B,H,W] fp32: the winner's disparity, bit for bit; 0.0 where nothing landed (a hole).  src (int [B,H,W], may be NULL):
 *     the winner's left column, -1 for a hole.  right must not be dl (ECM_EINVAL).
 * Fed to ecm_lr_check_fwd as dr (mirrored = 0), every candidate samples only columns it wrote to itself, so r >= d there: the
 * error is r - d and kind 2 does not occur; what the check then marks are the occlusions that the left map's own geometry implies.
 * One launch, a workgroup per row at a time, one 8-byte LDS word per column.  The only atomics are integer maxima in LDS: the
 * result does not depend on the order of arrival and is bit-reproducible.  B, H, W >= 1 and non-null dl, right, else ECM_EINVAL;
 * W > ecm_disp_splat_max_width() or B * H >= 2^31: ECM_EUNSUP, before any launch.  ecm_disp_splat_max_width is a size query (no
 * GPU). */
int ecm_disp_splat_max_width(void);
int ecm_disp_splat_fwd(const float* dl, float* right, int* src, int B, int H, int W, void* stream);

/* Harness loss + metrics (train.py:162,172-174; train_kitti.py:205-216) over n = B*H*W pixels; mask = 0 < gt < maxdisp.
 * out8 (device): [loss, #mask, epe(p3), err3(p3) in %, mean smooth-L1 of p1, p2, p3, 0];
 * loss = w1*m1 + w2*m2 + w3*m3 (reference weights 0.5 / 0.7 / 1.0).  Empty mask -> NaN (as the reference's empty mean).
 * bwd: g_k = gloss[0] * w_k / #mask * clamp(p_k - gt, -1, 1) inside the mask, 0 outside (gloss: device scalar). */
long long ecm_stereo_loss_scratch_bytes(long long n);
int ecm_stereo_loss_fwd(const float* p1, const float* p2, const float* p3, const float* gt, float* out8,
                        void* scratch, long long scratch_bytes, long long n, float maxdisp,
                        float w1, float w2, float w3, void* stream);
int ecm_stereo_loss_bwd(const float* p1, const float* p2, const float* p3, const float* gt, const float* out8,
                        const float* gloss, float* g1, float* g2, float* g3, long long n, float maxdisp,
                        float w1, float w2, float w3, void* stream);

/* ---- opt-in bf16 inference of the 3-D aggregation stack (ops.aggregation_dtype; bf16_infer.hip on bf16_conv3d.h) -------
 * (Its GroupNorm is the two-stage forward above: ecm_gn3d_stats_bf16, ecm_gn3d_apply_bf16 / _f32_bf16.)
 * Forward only.  Volumes are contiguous bf16 NCDHW (unsigned short = the bf16 bit pattern), weights and GroupNorm
 * parameters fp32; products accumulate in fp32 and every output is rounded once to bf16 (round to nearest even, NaN stays
 * NaN).  No atomics: bit-reproducible.
 * Weight image: [Ci/8][28 tap slots][Co][8] bf16 packed from the fp32 weight -- transposed = 0: Conv3d w [Co,Ci,3,3,3];
 * transposed = 1: ConvTranspose3d w [Ci,Co,3,3,3] (taps grouped by output phase).  Ci % 8 == 0. */
long long ecm_conv3d_bf16_packed_elems(int Ci, int Co);
int ecm_conv3d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int transposed, void* stream);
/* Conv3d k3 pad 1 stride 1|2, no bias (cmfsm.py:49-58): y [B,Co,Do,Ho,Wo], Do = (D-1)/stride+1.  Ci, Co in {32, 64}. */
int ecm_conv3d_k3_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, unsigned short* y,
                           int B, int Ci, int Co, int D, int H, int W, int stride, void* stream);
/* ConvTranspose3d k3 stride 2 pad 1 output_padding 1, no bias (cmfsm.py:262-268): y [B,Co,2D,2H,2W].  Ci, Co in {32, 64}. */
int ecm_deconv3d_k3s2_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, unsigned short* y,
                               int B, int Ci, int Co, int D, int H, int W, void* stream);
/* The classifier tail (ecm_conv3d_c1_gn_fwd) reading a bf16 x: relu(GroupNorm(x)) -> Conv3d(32 -> 1) with fp32 output
 * y [B,1,D,H,W]; statistics from ecm_gn3d_stats_bf16. */
int ecm_conv3d_c1_gn_fwd_bf16(const unsigned short* x, const float* mean_rstd, const float* gamma, const float* beta,
                              const float* w, float* y, int B, int Ci, int D, int H, int W, void* stream);

/* ---- opt-in bf16 inference of the 2-D feature encoder (ops.encoder_dtype; bf16_encoder.hip) -----------------------------
 * (Its GroupNorm is the two-stage forward above: ecm_gn3d_stats_bf16, ecm_gn3d_apply_bf16_f32.)
 * Forward only; replaces the encoder's Conv2d / GroupNorm layers after the stem (cmfsm.py:126-236).  Maps are contiguous
 * bf16 NCHW (unsigned short = the bf16 bit pattern), weights fp32 parameters packed to a bf16 image; products accumulate in
 * fp32 and every output is rounded once (round to nearest even, NaN stays NaN).  No atomics: bit-reproducible.
 * Weight image: [Ci/16][k*k taps][Co][16] bf16 of w [Co,Ci,k,k], k in {1, 3}; Ci % 16 == 0 (0 elements otherwise). */
long long ecm_conv2d_bf16_packed_elems(int Ci, int Co, int k);
int ecm_conv2d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int k, void* stream);
/* Conv2d without bias (convbn, cmfsm.py:36-46; the 1x1 projections): k = 3 with padding = dilation, stride 1 (dilation
 * 1|2|4) or 2 (dilation 1); k = 1 with padding 0, stride 1|2.  y [B,Co,Ho,Wo], Ho = (H-1)/stride+1: bf16, or fp32 with
 * out_f32 = 1 (the layers whose result leaves the encoder).  Ci % 16 == 0, Co % 32 == 0; any H, W >= 1. */
int ecm_conv2d_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, void* y, int B, int Ci, int Co, int H, int W,
                        int k, int stride, int dil, int out_f32, void* stream);

/* ---- opt-in bf16 inference of the cmf refinement decoder (ops.decoder_dtype; bf16_decoder.hip) --------------------------
 * Forward only.  The decoder's 3x3 convolutions run on ecm_conv2d_bf16_fwd and its GroupNorms on the two-stage kernels
 * above; these are the two layers they do not cover.  Maps are contiguous NCHW, bf16 as its bit pattern; products accumulate
 * in fp32; no atomics: bit-reproducible.
 * ConvTranspose2d(Ci, Co, 3, stride 2, padding 1, output_padding 1, bias=True) of deconv_module_list (cmf.py:236-239):
 * weight image [Ci/16][9 taps][Co][16] bf16 of w [Ci,Co,3,3]; Ci % 16 == 0 and Co in {32, 64} (0 elements otherwise). */
long long ecm_deconv2d_bf16_packed_elems(int Ci, int Co);
int ecm_deconv2d_bf16_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, void* stream);
/* cmf.py:236-239: bf16 x [B,Ci,H,W] -> bf16 y [B,Co,2H,2W]; the fp32 bias is added to the fp32 accumulators and every output
 * is rounded once (round to nearest even, NaN stays NaN).  Ci % 16 == 0, Co in {32, 64}; any H, W >= 1. */
int ecm_deconv2d_k3s2_bias_bf16_fwd(const unsigned short* x, const unsigned short* wpacked, const float* bias, unsigned short* y,
                                    int B, int Ci, int Co, int H, int W, void* stream);
/* conv_out + crap (cmf.py:259-264): relu(Conv2d(Ci, 1, 3, 1, 1, bias=True)(x)) of a bf16 x
 * [B,Ci,H,W] written as fp32 y [B,1,H,W], rounded nowhere.  w is the fp32 parameter [1,Ci,3,3], rounded to bf16 as the
 * kernel stages it; bias fp32 [1].  Ci % 16 == 0, Ci <= 1024; any H, W >= 1. */
int ecm_conv2d_c1_bf16_fwd(const unsigned short* x, const float* w, const float* bias, float* y, int B, int Ci, int H, int W,
                           void* stream);

/* ---- opt-in split-bf16 products for the stride-2 3-D convolutions (ops.split_products; split_bf16.hip on bf16_conv3d.h) -
 * Forward and data gradient of the hourglass's stride-2 family: Conv3d k3 p1 s2 (conv1 / conv3, cmfsm.py:244-258) and
 * ConvTranspose3d k3 s2 p1 op1 (conv5 / conv6, cmfsm.py:262-268); each is the other's adjoint, so the two entries serve all
 * four.  Volumes and results are contiguous fp32 NCDHW.  Every fp32 operand is split by truncation into three bf16 terms
 * (x = x1 + x2 + x3, exact for |x| >= 2^-110; a non-finite x is (x, 0, 0)) and the six leading cross products accumulate in
 * fp32 on the bf16 matrix cores: fp32-equivalent results.  No atomics: bit-reproducible.
 * Weight image: [Ci/8][3 terms][28 tap slots][Co][8] bf16 (unsigned short = the bit pattern), split once by the pack entry --
 * transposed = 0: Conv3d w [Co,Ci,3,3,3] read as a convolution; transposed = 1: ConvTranspose3d w [Ci,Co,3,3,3] read as a
 * transposed convolution (taps grouped by output phase).  Ci % 8 == 0 (0 elements otherwise).
 * Ci, Co in {32, 64} and byte offsets inside one sample below 2^31; anything else returns ECM_EUNSUP. */
long long ecm_conv3d_split_packed_elems(int Ci, int Co);
int ecm_conv3d_split_pack_weight(const float* w, unsigned short* packed, int Ci, int Co, int transposed, void* stream);
/* cmfsm.py:244-258: y [B,Co,Do,Ho,Wo], Do = (D-1)/2+1.  Also the data gradient of ecm_deconv3d_k3s2_split_fwd. */
int ecm_conv3d_k3s2_split_fwd(const float* x, const unsigned short* wpacked, float* y,
                              int B, int Ci, int Co, int D, int H, int W, void* stream);
/* cmfsm.py:262-268: y [B,Co,Do,Ho,Wo] with each output extent 2n (output_padding 1) or 2n-1 (the data gradient of
 * ecm_conv3d_k3s2_split_fwd on an odd extent). */
int ecm_deconv3d_k3s2_split_fwd(const float* x, const unsigned short* wpacked, float* y,
                                int B, int Ci, int Co, int D, int H, int W, int Do, int Ho, int Wo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECM_HIP_H */
