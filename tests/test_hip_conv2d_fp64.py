"""The 2-D convolution kernels against fp64, on every tile path of csrc/conv2d_kernel.h (the seven conv2d_case_*.hip), the 2-D parts
of conv3d_wgrad.hip, conv_wino.hip (KD 1) and deconv3d.hip (KD 1), and conv2d_c1.hip.

Which instantiation of conv2d_mfma runs is decided silently by the shape (`c2_plan`, `c2_nt` against `c2_min_blocks()`), and so is
how many tiles a persistent weight-gradient worker walks (`wgrad_workers` with occ = 2) and whether a tile is ragged.  The case table
below names, for every path class and every edge inside a path, the smallest shape that reaches it; the host-side dispatch is
restated here in Python so that the mapping is asserted (tests/test_conv2d_geometry.py pins every constant to its source and asserts
`missing_classes() == []` on the CPU) instead of assumed.  All operations are reached through ecm_amd.ops as the model reaches them:
ops.conv2d (also with the asymmetric padding and explicit output size of the two class convolutions), ops.conv2d_planes,
ops.deconv2d_k3s2_bias, ops.conv2d_c1_relu, ops.channel_sum and their autograd.  The restated `c2_min_blocks` is the DEFAULT (1536);
ECM_C2_MIN_BLOCKS is read once per process by the library, so the GPU tests skip when the variable is set.

Yardstick (the one of test_hip_numerics.py, test_hip_groupnorm_fp64.py and test_hip_conv3d_fp64.py).  Reference: F.conv2d /
F.conv_transpose2d and autograd in fp64 on the CPU; operands from oracle.weights.seeded under a name per case, weights He-scaled.
Unit: the reference's OWN fp32 error, e32(q) = max |q32 - q64| over independent fp32 evaluations of the same expression: torch's on
the CPU, torch's on the device, and -- for the quantities a Winograd kernel produced only -- the plain-torch fp32 restatement of
F(2x2,3x3) of test_hip_conv3d_fp64.py, applied to the 2-D operands as a depth-1 volume (`wino2_*` below;
`test_winograd2d_restatement_is_the_convolution` shows it equal to the reference in fp64).  For what conv2d_mfma produced, a further
candidate is the operation in that kernel's own summation order, `chain_conv2d`: one chain per output over (chunk of CIC channels,
tap, channel of the chunk), KH * KW * Ci terms one after another, where torch's convolutions sum in blocks.  The 3-D test found that
order to matter at 864 terms (5.4 x torch's error, which K = 4 does not contain); the candidate therefore enters the unit of a
conv2d_mfma quantity whose chain has CHAIN_MIN_TERMS = 864 terms or more, and of no other.  Those are the data gradients of
m33_c4_small (128 -> 64 in the kernel's roles, 1152 terms), md2_c4_small (1152), m35_q_small (192 -> 32, 2880), m33_p_small
(480 -> 32, 4320) and the forward of md4_c4_small (900).  On the MI355X two of them needed it: gx of m33_c4_small is 1.318e-05 from
fp64 where torch's fp32 is 2.27e-06 away (ratio 1.23 without the candidate) and gx of m35_q_small 2.29e-05 against 3.47e-06 (1.39);
the fp32 chain lands at 1.32e-05 and 2.48e-05, the kernel's own distance.  No weight-gradient, Winograd, transposed or
one-output-channel path has that candidate.  `test_chain2d_restatement_is_the_convolution` shows it equal to the reference in fp64.
A kernel passes when  max|q_hip - q64| <= K * e32(q) + FLOOR * max|q64|  with K = 4, FLOOR = 2e-7, for q in {y, gx, gw, gb}.  With
fork=True, gx must meet the same bound against the fp64 value of dgrad + gskip.

ops.conv2d_c1_relu: the bias is drawn so that about half of the outputs are clamped.  An output whose fp64 pre-activation lies
within RELU_EPS = 1e-5 of zero is left out of the comparison of y, and the gradient of y handed to backward is zero there, because a
correct fp32 evaluation may disagree about the mask at such an output; `relu_boundary_share` (asserted <= 0.1 % per case, on the CPU
in tests/test_conv2d_geometry.py and again here) is the only exclusion.

Every case runs twice on fresh operands and every output must reproduce bit for bit (the kernels claim fixed-order reductions).
Operands differ between cases and all outputs of a case stay alive until it ends, so an element a kernel failed to write cannot
inherit the right value from recycled memory.

Each test prints `C2RATIO <path> <quantity> <ratio>` with ratio = |q_hip - q64| / (K * e32 + floor); DESIGN.md section 4 holds the
worst ratio per path and quantity as measured on the MI355X."""
import collections
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

from oracle.weights import seeded
from test_hip_conv3d_fp64 import DEV, FLOOR, K, cdiv, switches, wino_dgrad, wino_fwd, wino_wgrad, worker_runs

pytestmark = pytest.mark.gpu


# ---- the host-side dispatch, restated (tests/test_conv2d_geometry.py pins every constant to its source) -------------------------
TW = 32                                 # fp32_conv_stage.h: output columns per tile (conv2d_kernel.h, deconv3d.hip)
TWV, CT = 16, 32                        # conv3d_wgrad.hip: output pixels per tile row, channel tile
C2_MIN_BLOCKS = 1536                    # c2_min_blocks(), default
# dispatch_c2<KH, KW, STRIDE, DIL, COTS>: bit (1 << cot) set = the case is instantiated for that many channel tiles
C2_COTS = {(3, 3, 1, 1): 30, (3, 3, 1, 2): 20, (3, 3, 1, 4): 16, (3, 3, 2, 1): 30, (3, 5, 1, 1): 10, (1, 1, 1, 1): 22, (1, 1, 2, 1): 22}
C2_NT_K11 = {1: 4, 2: 2, 4: 2}          # 1x1: C2_GO(cot, NT, 8)
C2_NT = {1: (8, 4), 2: (4, 2), 3: (2, 2), 4: (2, 1)}     # KH * KW > 1: (NT when c2_nt reaches it, NT otherwise); CIC 4
WGRAD_WORKERS, WGRAD_OCC2D = 256, 2
# WG2(KH, KW, S, DL, TH) -> launch_wgrad<S, 1, TH, 1, KH, KW, DL>
WG2_TH = {(3, 3, 1, 1): 16, (3, 3, 1, 2): 16, (3, 3, 1, 4): 16, (3, 3, 2, 1): 8, (3, 5, 1, 1): 16, (1, 1, 1, 1): 16, (1, 1, 2, 1): 8}
WGW_INST = (1, 16, 1)                   # launch_wgrad_wino<TD, TH, KD>
WINO_CIC2 = 4
WINO_INST = (1, 1, 2, WINO_CIC2)        # launch_wino<KD, TD, TR, CIC>
WINO_BLOCK = 32                         # consecutive 2x2 tiles per workgroup (x TR)
WINO2D_MIN_CI = 32                      # ops.WINO2D_MIN_CI, default
DECONV_TH, DECONV_CIC = 4, 4            # launch_deconv<CO_TILES, 4, 1[, true]>
C1_TX, C1_TY, C1_CC, C1_SUB, C1_CHUNK = 64, 32, 4, 4, 16384
CHAIN_MIN_TERMS = 864                   # module docstring
RELU_EPS, RELU_SHARE = 1e-5, 1e-3


def c2_plan(Ci, Co, kh, kw):
    """c2_plan of conv2d_kernel.h"""
    cot = 1 if Co <= 32 else 2 if Co <= 64 else 3 if (kh * kw != 1 and Co % 96 == 0 and Co % 128 != 0) else 4
    cic = 8 if kh * kw == 1 else 4
    return dict(cot=cot, cic=cic, groups=cdiv(Co, cot * 32), cip=cdiv(Ci, cic) * cic)


def c2_nt(cols_x_groups, Ho, max_nt):
    nt = max_nt
    while nt > 1:
        if cols_x_groups * cdiv(Ho, 4 * nt) >= C2_MIN_BLOCKS:
            return nt
        nt >>= 1
    return 1


def ops_cot(Co, kh, kw):
    """ops._cot"""
    if Co <= 32:
        return 1
    if Co <= 64:
        return 2
    return 3 if (kh * kw != 1 and Co % 96 == 0 and Co % 128 != 0) else 4


def ops_c2_cases():
    """ops._C2_CASES, from the COTS masks"""
    return {k: {cot for cot in (1, 2, 3, 4) if m >> cot & 1} for k, m in C2_COTS.items()}


def conv2d_supported(Ci, Co, kh, kw, stride, dil):
    """ops.conv2d_supported"""
    cots = ops_c2_cases().get((kh, kw, stride, dil))
    if cots is None or ops_cot(Co, kh, kw) not in cots:
        return False
    if stride == 1:
        return ops_cot(Ci, kh, kw) in cots
    if kh == 3:
        return Ci <= 64 and Co % 4 == 0
    return ops_cot(Ci, 1, 1) in ops_c2_cases()[(1, 1, 1, 1)]


def wino_ok(plane, winograd=True):
    """ops._wino_ok on the trailing (P,) h, w of x"""
    vol = 1
    for n in plane:
        vol *= n
    return winograd and plane[-1] >= 2 and vol * 128 <= 0x80000000


def c2_fwd(B, Ci, Co, Ho, Wo, kh, kw, stride, dil):
    """ecm_conv2d_fwd_ex -> dispatch_c2 -> launch_c2<COT, NT, CIC, ...>: the instantiation, its grid, chunk count, raggedness."""
    mask = C2_COTS.get((kh, kw, stride, dil))
    assert mask is not None, "ECM_EUNSUP"
    p = c2_plan(Ci, Co, kh, kw)
    cot = p["cot"]
    assert mask >> cot & 1, "ECM_EUNSUP"
    cg = B * cdiv(Wo, TW) * p["groups"]
    if kh * kw == 1:
        nt, chooses, large = C2_NT_K11[cot], False, False
    else:
        big, small = C2_NT[cot]
        if cot == 1 and stride != 1:
            big = small                 # 8 rows per wave at stride 2 is not instantiated
        chooses = big != small
        large = chooses and c2_nt(cg, Ho, big) >= big
        nt = big if large else small
    TH = 4 * nt
    return dict(inst=(cot, nt, p["cic"]), case=(kh, kw, stride, dil), chooses=chooses, large=large, TH=TH, groups=p["groups"],
                nblk=B * cdiv(Ho, TH) * cdiv(Wo, TW), chunks=p["cip"] // p["cic"], part_chunk=Ci % p["cic"] != 0,
                ragged=(Ho % TH != 0, Wo % TW != 0), co_guard=Co % (cot * 32) != 0, terms=kh * kw * Ci, Ci=Ci, Co=Co)


def wgrad_workers(Ci, Co, ntiles, occ):
    ytiles = cdiv(Ci, CT) * cdiv(Co, CT)
    return min(max(1, WGRAD_WORKERS * occ // ytiles), ntiles)


def wg2_geom(B, Ci, Co, Ho, Wo, kh, kw, stride, dil):
    """ecm_conv2d_wgrad_ex -> launch_wgrad<S, 1, TH, 1, KH, KW, DL> for gw [Co, Ci, kh, kw] over the output grid Ho x Wo."""
    TH = WG2_TH[(kh, kw, stride, dil)]
    assert TH == (16 if stride == 1 else 8)                     # ntiles2d_ex sizes the scratch by the stride alone
    ntiles = B * cdiv(Ho, TH) * cdiv(Wo, TWV)
    P = wgrad_workers(Ci, Co, ntiles, WGRAD_OCC2D)
    return dict(kind=(kh, kw, stride, dil), inst=(stride, 1, TH, 1, kh, kw, dil), ntiles=ntiles, P=P, runs=worker_runs(P, ntiles),
                ragged=(Ho % TH != 0, Wo % TWV != 0), ragged_ch=(Ci % CT != 0, Co % CT != 0))


def wgw_geom(B, Ci, Co, planes, H, W):
    """ecm_conv_wino_wgrad(kd 1) -> launch_wgrad_wino<1, 16, 1> on B x planes planes of H x W."""
    TD, TH, _ = WGW_INST
    ntiles = B * cdiv(planes, TD) * cdiv(H, TH) * cdiv(W, TWV)
    P = wgrad_workers(Ci, Co, ntiles, WGRAD_OCC2D)
    return dict(kind="wino", inst=WGW_INST, ntiles=ntiles, P=P, runs=worker_runs(P, ntiles), ragged=(H % TH != 0, W % TWV != 0),
                ragged_ch=(Ci % CT != 0, Co % CT != 0), H=H, W=W)


def wino_geom(B, Ci, Co, planes, H, W):
    """launch_wino<1, 1, 2, WINO_CIC2> for x [B, Ci, (planes,) H, W] -> Co channels."""
    KD, TD, TR, CIC = WINO_INST
    tiles_wt = (W + 1) // 2
    ntile = ((H + 1) // 2) * tiles_wt
    return dict(tiles_wt=tiles_wt, ntile=ntile, tblocks=cdiv(ntile, WINO_BLOCK * TR), nchunks=cdiv(Ci, CIC), groups=cdiv(Co, 32),
                Ci=Ci, Co=Co, H=H, W=W, planes=planes)


def deconv_geom(B, Ci, Co, H, W, Ho, Wo, bias):
    """ecm_deconv2d_k3s2_fwd / _bias_fwd on x [B, Ci, H, W] -> [B, Co, Ho, Wo] (each extent 2n or 2n - 1)."""
    assert Ci % 4 == 0 and 1 <= Co <= 64 and 2 * H - 1 <= Ho <= 2 * H and 2 * W - 1 <= Wo <= 2 * W, "ECM_EUNSUP"
    return dict(inst=(2 if Co > 32 else 1, DECONV_CIC, 1) + ((True,) if bias else ()), nblk=B * cdiv(H, DECONV_TH) * cdiv(W, TW),
                parity=(Ho % 2, Wo % 2), ragged=(H % DECONV_TH != 0, W % TW != 0), bias=bias, chunks=Ci // DECONV_CIC)


def c1_strips(H):
    return cdiv(H, C1_TY * C1_SUB)


def c1_geom(B, Ci, H, W):
    return dict(tiles=B * cdiv(H, C1_TY) * cdiv(W, C1_TX), workers=B * c1_strips(H) * cdiv(W, C1_TX), strips=c1_strips(H),
                part_chunk=Ci % C1_CC != 0, Ci=Ci, H=H, W=W)


def chsum_geom(B, Cc, HW):
    return dict(chunks=cdiv(HW, C1_CHUNK), vec=HW % 4 == 0)


# ---- the case table ------------------------------------------------------------------------------------------------------------
# op: "conv" = ops.conv2d; "planes" = ops.conv2d_planes on [B, Ci, P, H, W]; "deconvb" = ops.deconv2d_k3s2_bias; "c1" =
# ops.conv2d_c1_relu; "chsum" = ops.channel_sum on [B, Ci, H, W].  grads: "all" = forward + backward for every operand, "w" = the
# weight gradient alone (x does not require a gradient), "none" = forward alone (the large-tile cases: at most 12 input channels).
# wino / ww: ops.WINOGRAD / ops.WINOGRAD_WGRAD for the case; min_ci: ops.WINO2D_MIN_CI for the case (None = the default, 32);
# cls: "P" / "Q" = the padding and output size of the class convolutions of the collapsed cost volume (ops.costvol_conv3d).
Case = collections.namedtuple("Case", "op B Ci Co H W k stride dil grads wino ww min_ci fork frozen P cls",
                              defaults=((3, 3), 1, 1, "all", False, False, None, False, False, 0, None))


def _cv(B, Ci, Co, H, W, k=(3, 3), stride=1, dil=1, grads="all", **kw):
    return Case("conv", B, Ci, Co, H, W, k, stride, dil, grads, **kw)


def _wn(B, Ci, Co, H, W, **kw):
    return Case("conv", B, Ci, Co, H, W, wino=True, ww=True, min_ci=1, **kw)


MFMA = {
    # 3x3 / stride 1 / dilation 1 (COTS 1 2 3 4); direct weight gradient <1,1,16,1,3,3,1> (ops.WINOGRAD off)
    "m33_stem": _cv(1, 3, 8, 5, 9),                                     # <1,4,4>; one block; Ci % CIC != 0: empty-descriptor plane
    "m33_c1_two_chunks": _cv(1, 8, 32, 37, 70),                         # <1,4,4>; 9 blocks: unequal runs per XCD
    "m33_c1_flat": _cv(2, 4, 32, 16, 32),                               # nothing ragged
    "m33_c2_small": _cv(1, 12, 40, 19, 33),                             # <2,2,4>; 3 chunks; Co = 40 does not fill the tile
    "m33_c3_small": _cv(1, 8, 96, 9, 33),                               # <3,2,4>
    "m33_c4_small": _cv(1, 64, 128, 10, 35),                            # <4,1,4>; data gradient 128 -> 64 on <2,2,4>, 1152 terms
    "m33_groups": _cv(1, 4, 160, 6, 34),                                # cot 4, two groups, the second holds 32 of 128 channels
    "m33_c1_large": _cv(4, 4, 8, 600, 641, grads="none"),               # <1,8,4>: 4 * 21 * 19 = 1596 blocks, H and W ragged
    "m33_c1_large_flat": _cv(4, 4, 4, 768, 512, grads="none"),          # <1,8,4>: 4 * 16 * 24 = 1536 blocks, nothing ragged
    "m33_c2_large": _cv(4, 4, 33, 297, 641, grads="none"),              # <2,4,4>: 84 * 19 = 1596
    "m33_c4_large": _cv(4, 4, 65, 149, 641, grads="none"),              # <4,2,4>: 84 * 19 = 1596
    # 3x3 / dilation 2 (COTS 2 4) and 4 (COTS 4)
    "md2_c2_small": _cv(1, 36, 64, 11, 37, dil=2),                      # <2,2,4>; 9 chunks
    "md2_c4_small": _cv(1, 64, 128, 9, 34, dil=2),                      # <4,1,4>; data gradient on <2,2,4>
    "md2_c2_large": _cv(4, 4, 33, 297, 641, dil=2, grads="none"),
    "md2_c4_large": _cv(4, 4, 65, 149, 641, dil=2, grads="none"),
    "md4_c4_small": _cv(1, 100, 72, 13, 35, dil=4),                     # <4,1,4> both ways; 900 terms forward
    "md4_c4_large": _cv(4, 4, 65, 149, 641, dil=4, grads="none"),
    # 3x3 / stride 2 (COTS 1 2 3 4); data gradient = ecm_deconv2d_k3s2_fwd
    "ms2_c1": _cv(1, 8, 32, 10, 70, stride=2),                          # <1,4,4> (the only cot-1 tile at stride 2); H, W even
    "ms2_c2_small": _cv(1, 40, 64, 9, 67, stride=2),                    # <2,2,4>; deconv<2,4,1>; H, W odd: 2n - 1
    "ms2_c3_small": _cv(2, 8, 96, 14, 33, stride=2),                    # <3,2,4>; deconv<1,4,1>; H even, W odd
    "ms2_c4_small": _cv(1, 64, 128, 13, 66, stride=2),                  # <4,1,4>; deconv<2,4,1>; H odd, W even
    "ms2_c2_large": _cv(4, 4, 33, 593, 1281, stride=2, grads="none"),   # <2,4,4>: Ho 297, Wo 641
    "ms2_c4_large": _cv(4, 4, 65, 297, 1281, stride=2, grads="none"),   # <4,2,4>: Ho 149, Wo 641
    # 3x5 (COTS 1 3): same-style padding (1, 2), and the Q class convolution: pad_left 4, Wo = W + 2
    "m35_c1_small": _cv(1, 8, 16, 7, 35, k=(3, 5)),                     # <1,4,4>
    "m35_c1_large": _cv(4, 4, 8, 600, 641, k=(3, 5), grads="none"),     # <1,8,4>
    "m35_q_small": _cv(1, 32, 192, 6, 11, k=(3, 5), cls="Q"),           # <3,2,4>, 2 groups; data gradient 192 -> 32: 2880 terms
    "m35_q_large": _cv(1, 4, 192, 189, 1008, k=(3, 5), cls="Q", grads="none"),    # 2 * 24 * 32 = 1536 workgroups, H and Wo ragged
    # the P class convolution: 3x3, 32 -> 15 * 32, cot 3, 5 groups
    "m33_p_small": _cv(1, 32, 480, 6, 11, cls="P"),                     # data gradient 480 -> 32: 4320 terms
    "m33_p_large": _cv(1, 4, 480, 107, 700, cls="P", grads="none"),     # 5 * 14 * 22 = 1540 workgroups, H and W ragged
    # 1x1, stride 1 and 2 (COTS 1 2 4); CIC 8
    "m11_c1": _cv(1, 8, 32, 9, 33, k=(1, 1)),                           # <1,4,8>, one chunk
    "m11_c2": _cv(1, 20, 64, 17, 35, k=(1, 1)),                         # <2,2,8>; 3 chunks, the last one half empty
    "m11_c4": _cv(2, 64, 128, 7, 40, k=(1, 1)),                         # <4,2,8>; data gradient on <2,2,8>
    "m11s2_c1": _cv(1, 16, 32, 9, 35, k=(1, 1), stride=2),              # zero insertion: H, W odd
    "m11s2_c2": _cv(1, 40, 64, 10, 66, k=(1, 1), stride=2),             # H, W even
    "m11s2_c4": _cv(1, 64, 128, 11, 34, k=(1, 1), stride=2),            # H odd, W even
}
WGRAD = {
    # persistent schedules of conv3d_wgrad_mfma<S,1,TH,1,KH,KW,DL>: P = min(512 / ytiles, ntiles) < ntiles
    "g33_xcd": _cv(1, 128, 128, 90, 90, grads="w"),                     # 16 channel tiles: P = 32, 36 tiles: XCD runs of 5 and 4
    "g33_strided": _cv(2, 40, 72, 100, 100, grads="w"),                 # 6 channel tiles (ragged): P = 85, 98 tiles
    "gd2_xcd": _cv(1, 128, 128, 90, 90, dil=2, grads="w"),
    "gd2_strided": _cv(2, 40, 72, 100, 100, dil=2, grads="w"),
    "gd4_xcd": _cv(1, 128, 128, 90, 90, dil=4, grads="w"),
    "gd4_strided": _cv(1, 72, 100, 100, 100, dil=4, grads="w"),         # 12 channel tiles: P = 42, 49 tiles
    "gs2_xcd": _cv(1, 128, 128, 90, 180, stride=2, grads="w"),          # Ho 45, Wo 90: 36 tiles of 8 x 16
    "gs2_strided": _cv(2, 40, 72, 100, 200, stride=2, grads="w"),       # Ho 50, Wo 100: 98 tiles
    "g35_xcd": _cv(1, 128, 32, 170, 198, k=(3, 5), cls="Q", grads="w"),           # 4 channel tiles: P = 128, 11 * 13 = 143 tiles
    "g35_strided": _cv(1, 128, 96, 100, 100, k=(3, 5), grads="w"),      # 12 channel tiles: P = 42, 49 tiles
    "g11_xcd": _cv(1, 128, 128, 90, 90, k=(1, 1), grads="w"),
    "g11_strided": _cv(1, 72, 100, 100, 100, k=(1, 1), grads="w"),
    "g11s2_xcd": _cv(1, 128, 128, 90, 180, k=(1, 1), stride=2, grads="w"),
    "g11s2_strided": _cv(1, 72, 100, 100, 200, k=(1, 1), stride=2, grads="w"),
    # launch_wgrad_wino<1,16,1>
    "gw_xcd": _cv(1, 128, 128, 90, 90, grads="w", wino=True, ww=True),
    "gw_strided": _cv(2, 40, 72, 100, 100, grads="w", wino=True, ww=True),
}
WINO = {
    # conv_wino<1,1,2,4> forward and data gradient (ops.WINO2D_MIN_CI = 1), launch_wgrad_wino<1,16,1>
    "w_ci2_w2": _wn(1, 2, 8, 3, 2),                                     # one part chunk; W = 2
    "w_ci4_w3": _wn(1, 4, 4, 4, 3),                                     # one full chunk; W = 3; H even
    "w_ci6_co40_w127": _wn(1, 6, 40, 5, 127),                           # two chunks; second channel group of 8; 64 tiles per row
    "w_ci3_co480": _wn(1, 3, 480, 6, 7),                                # part chunk of 3; 15 groups; data gradient over 120 chunks
    "w_w128": _wn(1, 8, 8, 7, 128),
    "w_w129": _wn(2, 16, 16, 8, 129),                                   # 65 tiles per row
    "w_rows_wrap": _wn(1, 4, 8, 49, 6),                                 # 75 tiles of 3 per row: a block of 64 spans rows, ends ragged
    "w_fork_odd": _wn(1, 32, 32, 7, 35, fork=True),
    "w_fork_co40": _wn(1, 8, 40, 6, 67, fork=True),
    "w_fresh_pack": _wn(1, 32, 64, 6, 34, frozen=True),
    "w_planes_p4": Case("planes", 1, 8, 40, 5, 9, wino=True, ww=True, P=4),
    "w_planes_p16": Case("planes", 1, 4, 8, 6, 7, wino=True, ww=True, P=16, fork=True),
    # forward and data gradient on different kernels in one autograd call, at the default WINO2D_MIN_CI
    "x_direct_fwd_wino_bwd": _cv(1, 8, 32, 9, 35, wino=True, ww=True),  # Ci < 32 <= Co
    "x_wino_fwd_direct_bwd": _cv(1, 32, 8, 9, 35, wino=True, ww=True),  # Co < 32 <= Ci
}
DECODER = {
    # ops.deconv2d_k3s2_bias: launch_deconv<1|2,4,1,true>; data gradient on the stride-2 conv2d_mfma; role-exchanged <2,1,8,1,3,3,1>
    "db_96_32": Case("deconvb", 1, 96, 32, 5, 35),                      # data gradient 32 -> 96: cot 3
    "db_96_64": Case("deconvb", 1, 96, 64, 6, 33),
    "db_8_40": Case("deconvb", 2, 8, 40, 7, 9),
    "db_persistent": Case("deconvb", 2, 96, 64, 41, 120),               # 6 channel tiles: P = 85, 96 tiles; gb over 2 chunks of 16384
    "db_4_32_one_chunk": Case("deconvb", 1, 4, 32, 5, 33),              # Ci = CIC: the chunk loop without a prefetch; H, W ragged
    "ch_scalar": Case("chsum", 2, 5, 0, 7, 9),                          # HW % 4 != 0: scalar loads, one chunk
    "ch_chunks": Case("chsum", 1, 3, 0, 131, 127),                      # 16637 elements: a second chunk of 253
    # ops.conv2d_c1_relu: 64 x 32 tiles, 4 channels per step, strips of 4 tiles in the weight gradient
    "c1_ci5_w1": Case("c1", 1, 5, 1, 33, 1),
    "c1_ci7_h1": Case("c1", 1, 7, 1, 1, 63),
    "c1_ci96_w64": Case("c1", 1, 96, 1, 31, 64),
    "c1_ci4_w65": Case("c1", 2, 4, 1, 32, 65),
    "c1_ci96_w65": Case("c1", 1, 96, 1, 33, 65),
    "c1_strips": Case("c1", 2, 8, 1, 130, 70),                          # two strips (the second holds one tile), two tile columns
}
CASES = {**MFMA, **WGRAD, **WINO, **DECODER}


def geometry(c):
    """pad_top, pad_left, Ho, Wo of a "conv" case as ops.conv2d derives them (or as ops.costvol_conv3d passes them)."""
    kh, kw = c.k
    if c.cls == "Q":
        return 1, 4, c.H, c.W + 2
    pt, pl = c.dil * (kh - 1) // 2, c.dil * (kw - 1) // 2
    return (pt, pl, (c.H + 2 * pt - c.dil * (kh - 1) - 1) // c.stride + 1, (c.W + 2 * pl - c.dil * (kw - 1) - 1) // c.stride + 1)


def wino_flags(c):
    """(wino_f, wino_b, same) of ops.Conv2dG.forward"""
    kh, kw = c.k
    pt, pl, Ho, Wo = geometry(c)
    same = (kh, kw, c.stride, c.dil, pt, pl) == (3, 3, 1, 1, 1, 1) and (Ho, Wo) == (c.H, c.W)
    m = WINO2D_MIN_CI if c.min_ci is None else c.min_ci
    ok = wino_ok((c.H, c.W), c.wino)
    return ok and same and c.Ci >= m, ok and same and c.Co >= m, same


def launches(c):
    """Every kernel launch a case makes, as (quantity, family, geometry): what the autograd functions of ops dispatch to."""
    B, Ci, Co, H, W = c.B, c.Ci, c.Co, c.H, c.W
    if c.op == "chsum":
        return [("gb", "chsum", chsum_geom(B, Ci, H * W))]
    if c.op == "c1":
        g = c1_geom(B, Ci, H, W)
        return [("y", "c1", g), ("gx", "c1", g), ("gw", "c1", g), ("gb", "c1", g)]
    if c.op == "deconvb":
        return [("y", "deconv", deconv_geom(B, Ci, Co, H, W, 2 * H, 2 * W, True)),
                ("gx", "c2", dict(c2_fwd(B, Co, Ci, H, W, 3, 3, 2, 1), dgrad=True)),
                ("gw", "wg2", dict(wg2_geom(B, Co, Ci, H, W, 3, 3, 2, 1), exchanged=True)),
                ("gb", "chsum", chsum_geom(B, Co, 4 * H * W))]
    if c.op == "planes":
        assert wino_ok((c.P, H, W), c.wino) and c.ww
        out = [("y", "wino", wino_geom(B, Ci, Co, c.P, H, W))]
        if c.grads == "all":
            out += [("gx", "wino", dict(wino_geom(B, Co, Ci, c.P, H, W), add=c.fork, fresh=c.frozen)),
                    ("gw", "wgw", wgw_geom(B, Ci, Co, c.P, H, W))]
        return out
    kh, kw = c.k
    pt, pl, Ho, Wo = geometry(c)
    wf, wb, same = wino_flags(c)
    out = [("y", "wino", wino_geom(B, Ci, Co, 1, H, W)) if wf else ("y", "c2", c2_fwd(B, Ci, Co, Ho, Wo, kh, kw, c.stride, c.dil))]
    if c.grads == "all":
        if wb:
            out.append(("gx", "wino", dict(wino_geom(B, Co, Ci, 1, H, W), add=c.fork, fresh=c.frozen)))
        elif c.stride == 1:
            out.append(("gx", "c2", dict(c2_fwd(B, Co, Ci, H, W, kh, kw, 1, c.dil), dgrad=True)))
        elif kh == 3:
            out.append(("gx", "deconv", deconv_geom(B, Co, Ci, Ho, Wo, H, W, False)))
        else:
            out.append(("gx", "c2", dict(c2_fwd(B, Co, Ci, Ho, Wo, 1, 1, 1, 1), dgrad=True, zero_insert=(H % 2, W % 2))))
    if c.grads != "none":
        if same and wino_ok((H, W), c.wino) and c.ww:
            out.append(("gw", "wgw", wgw_geom(B, Ci, Co, 1, H, W)))
        else:
            out.append(("gw", "wg2", wg2_geom(B, Ci, Co, Ho, Wo, kh, kw, c.stride, c.dil)))
    return out


def path_name(q, fam, g):
    if fam == "c1":
        return {"y": "c1_fwd", "gx": "c1_dgrad", "gw": "c1_wgrad", "gb": "c1_wgrad"}[q]
    if fam == "chsum":
        return "channel_sum"
    if fam == "c2":
        return "c2_k%d%d_s%d_d%d" % g["case"] + "<%d,%d,%d>" % g["inst"] + (":dgrad" if g.get("dgrad") else "") + \
               ("+zero_insert" if "zero_insert" in g else "")
    if fam == "deconv":
        return "deconv<%s>" % ",".join(str(v).lower() for v in g["inst"])
    if fam == "wino":
        return "wino<%d,%d,%d,%d>" % WINO_INST + ("+add" if g.get("add") else "")
    if fam == "wgw":
        return "wgrad_wino<%d,%d,%d>" % g["inst"]
    if fam == "wg2":
        return "wgrad<%d,%d,%d,%d,%d,%d,%d>" % g["inst"] + (":exchanged" if g.get("exchanged") else "")
    raise KeyError(fam)


def all_c2_instantiations():
    """(case, (COT, NT, CIC)) for everything dispatch_c2 can return."""
    out = []
    for case, mask in C2_COTS.items():
        kh, kw, stride, _ = case
        for cot in (1, 2, 3, 4):
            if not mask >> cot & 1:
                continue
            if kh * kw == 1:
                out.append((case, (cot, C2_NT_K11[cot], 8)))
                continue
            big, small = C2_NT[cot]
            if cot == 1 and stride != 1:
                big = small
            out += [(case, (cot, nt, 4)) for nt in sorted({big, small})]
    return out


def missing_classes():
    """The path classes (the issue's list, the case table) that NO case reaches under the restated dispatch."""
    L = [(name, CASES[name], q, fam, g) for name in CASES for q, fam, g in launches(CASES[name])]
    c2 = [g for _, _, _, fam, g in L if fam == "c2"]
    c2f = [g for g in c2 if not g.get("dgrad")]
    want = {}
    for case, inst in all_c2_instantiations():
        want["conv2d_mfma forward %s %s" % (case, inst)] = any(g["case"] == case and g["inst"] == inst for g in c2f)
    for cot in (1, 2, 4):
        big = C2_NT[cot][0]
        want["conv2d_mfma <%d,%d,4>: Ho %% TH != 0 and Wo %% 32 != 0" % (cot, big)] = any(
            g["inst"] == (cot, big, 4) and g["large"] and all(g["ragged"]) for g in c2f)
    want["conv2d_mfma large NT, nothing ragged"] = any(g["large"] and not any(g["ragged"]) for g in c2f)
    for n in (1, 2, 3):
        want["conv2d_mfma: %s chunk(s) of CIC" % (n if n < 3 else ">= 3")] = any(g["chunks"] == n if n < 3 else g["chunks"] >= 3 for g in c2f)
    want["conv2d_mfma: Ci % CIC != 0 at 3 channels"] = any(g["part_chunk"] and g["Ci"] == 3 for g in c2f)
    want["conv2d_mfma: Co does not fill the last group"] = any(g["co_guard"] for g in c2f)
    want["conv2d_mfma: groups > 1"] = any(g["groups"] > 1 for g in c2f)
    want["conv2d_mfma: nblk < 8"] = any(g["nblk"] < 8 for g in c2f)
    want["conv2d_mfma: nblk % 8 != 0 (unequal XCD runs)"] = any(g["nblk"] > 8 and g["nblk"] % 8 for g in c2f)
    for cls, co in (("Q", 192), ("P", 480)):
        k = [(c, g) for _, c, q, fam, g in L if fam == "c2" and q == "y" and c.cls == cls and c.Co == co]
        want["class convolution %s: cot 3, small" % cls] = any(g["inst"][0] == 3 and g["nblk"] * g["groups"] < 64 for _, g in k)
        want["class convolution %s: cot 3, >= 1536 workgroups, ragged" % cls] = any(
            g["inst"][0] == 3 and g["nblk"] * g["groups"] >= C2_MIN_BLOCKS and all(g["ragged"]) for _, g in k)
    want["class convolution P: 5 groups"] = any(g["groups"] == 5 and g["inst"][0] == 3 for g in c2f)
    # stride-1 data gradients on the flip-transposed weights
    for case in C2_COTS:
        if case[2] == 1:
            k = [g for g in c2 if g.get("dgrad") and g["case"] == case and "zero_insert" not in g]
            want["stride-1 data gradient %s" % (case,)] = bool(k)
            if bin(C2_COTS[case]).count("1") > 1:
                want["stride-1 data gradient %s with another cot than the forward" % (case,)] = any(
                    c2_plan(g["Co"], g["Ci"], case[0], case[1])["cot"] != g["inst"][0] for g in k)
    dec = [(q, g) for _, _, q, fam, g in L if fam == "deconv"]
    dg = [g for q, g in dec if not g["bias"]]
    for ct in (1, 2):
        want["stride-2 3x3 data gradient launch_deconv<%d,4,1>" % ct] = any(g["inst"] == (ct, 4, 1) for g in dg)
        want["ops.deconv2d_k3s2_bias launch_deconv<%d,4,1,true>" % ct] = any(g["inst"] == (ct, 4, 1, True) for q, g in dec)
    for par in ((0, 0), (1, 1), (0, 1), (1, 0)):
        want["stride-2 3x3 data gradient: H, W parity %s" % (par,)] = any(g["parity"] == par for g in dg)
    want["stride-2 3x3 data gradient: H % 4 and W % 32 ragged"] = any(all(g["ragged"]) for g in dg)
    want["ops.deconv2d_k3s2_bias: H % 4 and W % 32 ragged"] = any(all(g["ragged"]) for q, g in dec if g["bias"])
    for n in (1, 2, 3):         # the regimes of the shared chunk loop (fp32_conv_stage.h): no prefetch, one, a prefetch of a prefetch
        want["launch_deconv<.,4,1>: %s chunk(s) of CIC" % (n if n < 3 else ">= 3")] = any(g["chunks"] == n if n < 3 else g["chunks"] >= 3 for q, g in dec)
        for kk, cic in ((9, 4), (1, 8)):
            want["conv2d_mfma %s, CIC %d: %s chunk(s)" % ("3x3" if kk == 9 else "1x1", cic, n if n < 3 else ">= 3")] = any(
                g["case"][0] * g["case"][1] == kk and g["inst"][2] == cic and (g["chunks"] == n if n < 3 else g["chunks"] >= 3) for g in c2)
    zi = [g["zero_insert"] for g in c2 if "zero_insert" in g]
    for par in (0, 1):
        want["stride-2 1x1 data gradient: H %s" % ("odd" if par else "even")] = any(z[0] == par for z in zi)
        want["stride-2 1x1 data gradient: W %s" % ("odd" if par else "even")] = any(z[1] == par for z in zi)
    # weight gradients
    wg = [g for _, _, _, fam, g in L if fam in ("wg2", "wgw")]
    for kind in list(WG2_TH) + ["wino"]:
        k = [g for g in wg if g["kind"] == kind and not g.get("exchanged")]
        lab = "wgrad %s: " % (kind,)
        want[lab + "P == ntiles"] = any(g["P"] == g["ntiles"] for g in k)
        want[lab + "P < ntiles, P % 8 == 0, unequal XCD runs"] = any(g["P"] < g["ntiles"] and g["P"] % 8 == 0 and g["ntiles"] % 8 for g in k)
        want[lab + "P < ntiles, P % 8 != 0"] = any(g["P"] < g["ntiles"] and g["P"] % 8 for g in k)
        want[lab + "ragged channel tiles"] = any(all(g["ragged_ch"]) for g in k)
        want[lab + "Ho % TH and Wo % 16 ragged"] = any(all(g["ragged"]) for g in k)
    want["wgrad: role-exchanged, P < ntiles"] = any(g.get("exchanged") and g["P"] < g["ntiles"] for g in wg)
    # Winograd
    wino = [(c, q, g) for _, c, q, fam, g in L if fam == "wino"]
    wf = [g for _, q, g in wino if q == "y"]
    wd = [g for _, q, g in wino if q == "gx"]
    for w in (2, 3, 127, 128, 129):
        want["winograd: W = %d" % w] = any(g["W"] == w for g in wf)
    for par in (0, 1):
        want["winograd: H %s" % ("odd" if par else "even")] = any(g["H"] % 2 == par for g in wf)
    want["winograd: a block of 64 tiles spans rows and ends ragged"] = any(
        g["tiles_wt"] < 2 * WINO_BLOCK and g["ntile"] > 2 * WINO_BLOCK and g["ntile"] % (2 * WINO_BLOCK) for g in wf)
    for ci in (2, 4, 6, 3):
        want["winograd forward Ci = %d" % ci] = any(g["Ci"] == ci for g in wf)
    for co in (40, 480):
        want["winograd forward Co = %d" % co] = any(g["Co"] == co for g in wf)
    want["winograd data gradient + addend"] = any(g["add"] for g in wd)
    want["winograd data gradient without addend"] = any(not g["add"] for g in wd)
    want["winograd data gradient, layout packed afresh"] = any(g["fresh"] for g in wd)
    for p in (4, 16):
        want["ops.conv2d_planes: P = %d" % p] = any(c.op == "planes" and c.P == p for c, q, g in wino)
    want["Ci < WINO2D_MIN_CI <= Co at the default: direct forward, Winograd data gradient"] = any(
        c.min_ci is None and not wino_flags(c)[0] and wino_flags(c)[1] and c.grads == "all" for c in CASES.values() if c.op == "conv")
    want["Co < WINO2D_MIN_CI <= Ci at the default: Winograd forward, direct data gradient"] = any(
        c.min_ci is None and wino_flags(c)[0] and not wino_flags(c)[1] and c.grads == "all" for c in CASES.values() if c.op == "conv")
    # cmf decoder layers
    db = [c for c in CASES.values() if c.op == "deconvb"]
    want["deconv2d_k3s2_bias: Co <= 32"] = any(c.Co <= 32 for c in db)
    want["deconv2d_k3s2_bias: Co > 32"] = any(c.Co > 32 for c in db)
    want["deconv2d_k3s2_bias: Ci = 96, data gradient on cot 3"] = any(
        c.Ci == 96 and g["inst"][0] == 3 for _, c, q, fam, g in L if c.op == "deconvb" and fam == "c2")
    want["deconv2d_k3s2_bias: a small Ci"] = any(c.Ci <= 12 for c in db)
    ch = [g for _, _, _, fam, g in L if fam == "chsum"]
    want["channel_sum: one chunk"] = any(g["chunks"] == 1 for g in ch)
    want["channel_sum: several chunks"] = any(g["chunks"] > 1 for g in ch)
    want["channel_sum: scalar loads"] = any(not g["vec"] for g in ch)
    c1 = [g for _, _, q, fam, g in L if fam == "c1" and q == "y"]
    for ci in (5, 7, 96):
        want["conv2d_c1_relu: Ci = %d" % ci] = any(g["Ci"] == ci for g in c1)
    for w in (1, 63, 64, 65):
        want["conv2d_c1_relu: W = %d" % w] = any(g["W"] == w for g in c1)
    for h in (1, 31, 32, 33):
        want["conv2d_c1_relu: H = %d" % h] = any(g["H"] == h for g in c1)
    want["conv2d_c1_relu: more than one strip of 128 rows"] = any(g["strips"] > 1 and g["H"] % (C1_TY * C1_SUB) for g in c1)
    return sorted(k for k, ok in want.items() if not ok)


# ---- the restatements that enter the unit ---------------------------------------------------------------------------------------
def _embed(w):
    """[Co, Ci, 3, 3] as the centre depth tap of a [Co, Ci, 3, 3, 3] kernel"""
    w3 = w.new_zeros(w.shape[0], w.shape[1], 3, 3, 3)
    w3[:, :, 1] = w
    return w3


def wino2_fwd(x, w):
    """conv2d(x, w, stride 1, pad 1) by F(2x2,3x3): the 3-D test's restatement on a depth-1 volume (the depth taps 0 and 2 are zero)"""
    return wino_fwd(x.unsqueeze(2), _embed(w)).squeeze(2)


def wino2_dgrad(gy, w):
    return wino_dgrad(gy.unsqueeze(2), _embed(w)).squeeze(2)


def wino2_wgrad(x, gy):
    return wino_wgrad(x.unsqueeze(2), gy.unsqueeze(2))[:, :, 1]


def to_planes(x):
    """[B, C, P, h, w] -> [B * P, C, h, w]"""
    B, Cc, P, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(B * P, Cc, h, w)


def from_planes(y, B):
    BP, Cc, h, w = y.shape
    return y.reshape(B, BP // B, Cc, h, w).permute(0, 2, 1, 3, 4).contiguous()


def conv_ref(x, w, stride, dil, pt, pl, Ho, Wo):
    """The convolution with explicit top / left padding and output size through F.conv2d (the bottom / right padding follows)."""
    kh, kw = w.shape[-2:]
    H, W = x.shape[-2:]
    pb = (Ho - 1) * stride + dil * (kh - 1) + 1 - H - pt
    pr = (Wo - 1) * stride + dil * (kw - 1) + 1 - W - pl
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, None, stride, 0, dil)


def chain_conv2d(x, w, stride, dil, pt, pl, Ho, Wo, cic):
    """conv_ref as conv2d_mfma sums it: ONE chain per output element, acc <- acc + w * x one term after another over (chunk of
    `cic` input channels, tap, channel of the chunk), in the dtype of the operands."""
    B, Ci, H, W = x.shape
    kh, kw = w.shape[-2:]
    pb = max(0, (Ho - 1) * stride + dil * (kh - 1) + 1 - H - pt)
    pr = max(0, (Wo - 1) * stride + dil * (kw - 1) + 1 - W - pl)
    xp = F.pad(x, (pl, pr, pt, pb))
    acc = x.new_zeros(B, w.shape[0], Ho, Wo)
    for c0 in range(0, Ci, cic):
        for a in range(kh):
            for b in range(kw):
                for c in range(c0, min(c0 + cic, Ci)):
                    win = xp[:, c:c + 1, a * dil:a * dil + (Ho - 1) * stride + 1:stride, b * dil:b * dil + (Wo - 1) * stride + 1:stride]
                    acc = acc + w[:, c, a, b].view(1, -1, 1, 1) * win
    return acc


def flip_t(w):
    return w.flip(2, 3).transpose(0, 1)


def zero_insert(small, H, W):
    g = small.new_zeros(small.shape[0], small.shape[1], H, W)
    g[:, :, ::2, ::2] = small
    return g


# ---- operands, references ----------------------------------------------------------------------------------------------------------
def operands(name, c):
    """dict(x, w, b, G, Gs): the operands of a case (w, b, Gs None where the operation has none)."""
    n = "c2." + name
    if c.op == "chsum":
        return dict(x=seeded(n + ".x", c.B, c.Ci, c.H, c.W), w=None, b=None, G=None, Gs=None)
    if c.op == "c1":
        x = seeded(n + ".x", c.B, c.Ci, c.H, c.W)
        w = seeded(n + ".w", 1, c.Ci, 3, 3) * (2.0 / (9 * c.Ci)) ** 0.5
        b = seeded(n + ".b", 1) * 0.25                              # |b| << the spread of the pre-activation: about half are clamped
        pre = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
        keep = (pre.abs() >= RELU_EPS)
        return dict(x=x, w=w, b=b, G=seeded(n + ".G", c.B, 1, c.H, c.W) * keep, Gs=None, keep=keep, pre=pre)
    if c.op == "deconvb":
        return dict(x=seeded(n + ".x", c.B, c.Ci, c.H, c.W), w=seeded(n + ".w", c.Ci, c.Co, 3, 3) * (2.0 / (9 * c.Ci)) ** 0.5,
                    b=seeded(n + ".b", c.Co), G=seeded(n + ".G", c.B, c.Co, 2 * c.H, 2 * c.W), Gs=None)
    kh, kw = c.k
    _, _, Ho, Wo = geometry(c)
    plane = (c.P,) if c.op == "planes" else ()
    x = seeded(n + ".x", c.B, c.Ci, *plane, c.H, c.W)
    return dict(x=x, w=seeded(n + ".w", c.Co, c.Ci, kh, kw) * (2.0 / (kh * kw * c.Ci)) ** 0.5, b=None,
                G=None if c.grads == "none" else seeded(n + ".G", c.B, c.Co, *plane, Ho, Wo),
                Gs=seeded(n + ".Gs", *x.shape) if c.fork else None)


def relu_boundary_share(name):
    """(share of the outputs of a conv2d_c1_relu case within RELU_EPS of the ReLU's kink, share of clamped outputs): fp64, CPU."""
    o = operands(name, CASES[name])
    return 1.0 - float(o["keep"].double().mean()), float((o["pre"] < 0).double().mean())


def _forward(c, x, w, b):
    """The operation in the dtype and on the device of its operands, through torch's own kernels."""
    if c.op == "chsum":
        return x.sum((0, 2, 3))
    if c.op == "c1":
        return F.relu(F.conv2d(x, w, b, 1, 1))
    if c.op == "deconvb":
        return F.conv_transpose2d(x, w, b, 2, 1, 1)
    if c.op == "planes":
        return from_planes(F.conv2d(to_planes(x), w, None, 1, 1), x.shape[0])
    pt, pl, Ho, Wo = geometry(c)
    return conv_ref(x, w, c.stride, c.dil, pt, pl, Ho, Wo)


def _torch(c, o, dtype, device):
    cv = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype, copy=True)      # noqa: E731
    x, w, b = cv(o["x"]), cv(o["w"]), cv(o["b"])
    if c.op == "chsum":
        return {"gb": _forward(c, x, w, b)}
    if c.grads == "none":
        with torch.no_grad():
            return {"y": _forward(c, x, w, b)}
    x.requires_grad_(c.grads == "all")
    w.requires_grad_()
    if b is not None:
        b.requires_grad_()
    y = _forward(c, x, w, b)
    y.backward(cv(o["G"]))
    out = {"gw": w.grad}
    if c.grads == "all":
        out["y"] = y.detach()
        out["gx"] = x.grad if o["Gs"] is None else x.grad + cv(o["Gs"])
    if b is not None:
        out["gb"] = b.grad
    return out


def _wino32(c, o, which):
    """The fp32 Winograd restatement on the device for the quantities in `which`."""
    x, w = o["x"].to(DEV), o["w"].to(DEV)
    G = None if o["G"] is None else o["G"].to(DEV)
    B = x.shape[0]
    pl = c.op == "planes"
    out = {}
    if "y" in which:
        out["y"] = from_planes(wino2_fwd(to_planes(x), w), B) if pl else wino2_fwd(x, w)
    if "gx" in which:
        gx = from_planes(wino2_dgrad(to_planes(G), w), B) if pl else wino2_dgrad(G, w)
        out["gx"] = gx if o["Gs"] is None else gx + o["Gs"].to(DEV)
    if "gw" in which:
        out["gw"] = wino2_wgrad(to_planes(x), to_planes(G)) if pl else wino2_wgrad(x, G)
    return out


def _chain32(c, o, L):
    """The fp32 chain restatement on the device for the conv2d_mfma quantities whose chain has CHAIN_MIN_TERMS terms or more."""
    out = {}
    for q, fam, g in L:
        if fam != "c2" or g["terms"] < CHAIN_MIN_TERMS:
            continue
        cic = g["inst"][2]
        w = o["w"].to(DEV)
        if q == "y":
            pt, pl, Ho, Wo = geometry(c)
            out["y"] = chain_conv2d(o["x"].to(DEV), w, c.stride, c.dil, pt, pl, Ho, Wo, cic)
            continue
        G = o["G"].to(DEV)
        if c.op == "deconvb":                   # the stride-2 convolution of G by the weight read as Conv2d's [Ci, Co, 3, 3]
            gx = chain_conv2d(G, w, 2, 1, 1, 1, c.H, c.W, cic)
        elif "zero_insert" in g:
            gx = zero_insert(chain_conv2d(G, flip_t(w), 1, 1, 0, 0, G.shape[2], G.shape[3], cic), c.H, c.W)
        else:
            kh, kw = c.k
            pt, pl, _, _ = geometry(c)
            gx = chain_conv2d(G, flip_t(w), 1, c.dil, (kh - 1) * c.dil - pt, (kw - 1) * c.dil - pl, c.H, c.W, cic)
        out["gx"] = gx if o["Gs"] is None else gx + o["Gs"].to(DEV)
    return out


# ---- fixtures and helpers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ecm():
    if "ECM_C2_MIN_BLOCKS" in os.environ:
        pytest.skip("ECM_C2_MIN_BLOCKS is set: the library reads it once per process and the case table assumes the default 1536")
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


@contextlib.contextmanager
def min_ci(ecm, value):
    prev = ecm.ops.WINO2D_MIN_CI
    if value is not None:
        ecm.ops.WINO2D_MIN_CI = value
    try:
        yield
    finally:
        ecm.ops.WINO2D_MIN_CI = prev


def _hip(ecm, c, o):
    """The operation through ecm_amd.ops on fresh copies of the operands."""
    ops = ecm.ops
    d = lambda t: None if t is None else t.to(DEV)                   # noqa: E731
    x, w, b, G, Gs = d(o["x"]), d(o["w"]), d(o["b"]), d(o["G"]), d(o["Gs"])
    if c.op == "chsum":
        return {"gb": ops.channel_sum(x)}
    if c.grads != "none":
        x.requires_grad_(c.grads == "all")
        w.requires_grad_()
        if b is not None:
            b.requires_grad_()
    xa = None
    with (ops.frozen_weights() if c.frozen else contextlib.nullcontext()), (torch.no_grad() if c.grads == "none" else contextlib.nullcontext()):
        if c.op == "c1":
            y = ops.conv2d_c1_relu(x, w, b)
        elif c.op == "deconvb":
            y = ops.deconv2d_k3s2_bias(x, w, b)
        elif c.op == "planes":
            y = ops.conv2d_planes(x, w, fork=c.fork)
        elif c.cls is not None:                 # as ops.costvol_conv3d calls it: padding and output size spelled out
            y = ops.conv2d(x, w, 1, 1, *geometry(c))
        else:
            y = ops.conv2d(x, w, c.stride, c.dil, fork=c.fork)
        if c.fork:
            y, xa = y
            assert xa.data_ptr() == x.data_ptr()
    assert y.dtype == torch.float32 and y.is_contiguous()
    if c.grads == "none":
        return {"y": y}
    assert y.shape == G.shape
    if c.fork:
        torch.autograd.backward([y, xa], [G, Gs])
    else:
        y.backward(G)
    ops.join_side_streams()
    out = {"gw": w.grad}
    if c.grads == "all":
        out["y"], out["gx"] = y.detach(), x.grad
    if b is not None:
        out["gb"] = b.grad
    for k, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous(), k
    assert w.grad.shape == w.shape and (c.grads != "all" or x.grad.shape == x.shape) and (b is None or b.grad.shape == b.shape)
    return out


def _compare(label, paths, hip, q64, e32, fails, parts, keep=None):
    """Module-docstring rule for every quantity; prints the ratios, collects the failures (asserted after all prints)."""
    for k, got in hip.items():
        ref = q64[k]
        diff = (got.cpu().double() - ref).abs()
        if k == "y" and keep is not None:
            diff, ref = diff * keep, ref * keep
        err, scale = float(diff.max()), float(ref.abs().max())
        bound = K * e32[k] + FLOOR * scale
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"C2RATIO {paths[k]} {k} {ratio:.3f}   # {label}: err {err:.3e}, e32 {e32[k]:.3e} [{parts[k]}], max|ref| {scale:.3e}")
        if not err <= bound:                                     # (a NaN fails)
            fails.append(f"{label}: {k} on {paths[k]}: |hip - fp64| = {err:.3e} > {K} * {e32[k]:.3e} + {FLOOR} * {scale:.3e}"
                         f" (ratio {ratio:.2f})")


def _run_case(ecm, name):
    c = CASES[name]
    o = operands(name, c)
    L = launches(c)
    keep = o.get("keep")
    fails = []
    if keep is not None:
        share, clamped = relu_boundary_share(name)
        assert share <= RELU_SHARE, f"{name}: {share:.2%} of the outputs lie within {RELU_EPS} of the ReLU's kink"
        keep = keep.double()
    runs = None
    try:
        with switches(ecm, c.wino, c.ww), min_ci(ecm, c.min_ci):
            runs = [_hip(ecm, c, o) for _ in range(2)]
        q64 = _torch(c, o, torch.float64, "cpu")
        draws = [_torch(c, o, torch.float32, "cpu"), _torch(c, o, torch.float32, DEV)]
        paths, wq = {}, set()
        for q, fam, g in L:
            paths[q] = path_name(q, fam, g)
            if fam in ("wino", "wgw"):
                wq.add(q)
        wdraw = _wino32(c, o, wq) if wq else {}
        cdraw = _chain32(c, o, L)
        a, b = runs
        assert set(a) == set(q64) and set(a) <= set(paths), (sorted(a), sorted(q64), sorted(paths))
        e32, parts = {}, {}
        for k in a:
            cand = [d[k] for d in draws] + [d[k] for d in (wdraw, cdraw) if k in d]
            each = [(t.cpu().double() - q64[k]).abs() for t in cand]
            if k == "y" and keep is not None:
                each = [e * keep for e in each]
            each = [float(e.max()) for e in each]
            e32[k], parts[k] = max(each), " ".join("%.2e" % e for e in each)
        _compare(name, paths, a, q64, e32, fails, parts, keep)
        for k in a:
            if not torch.equal(a[k], b[k]):
                fails.append(f"{name}: {k} differs between two runs in {int((a[k] != b[k]).sum())} elements")
        ecm.ops.check_async_errors()
        assert not fails, "\n".join(fails)
    finally:
        del runs


# ---- the tests -------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_class():
    assert missing_classes() == []


RESTATEMENT_SHAPES = [(1, 3, 5, 5, 7), (2, 4, 3, 4, 2), (1, 2, 2, 3, 6)]            # odd / even H and W, W = 2, odd Ci


@pytest.mark.parametrize("shape", RESTATEMENT_SHAPES, ids=str)
def test_winograd2d_restatement_is_the_convolution(shape):
    """wino2_fwd / wino2_dgrad / wino2_wgrad in fp64 equal F.conv2d and its autograd in fp64 to 1e-12 of scale, on [B,C,H,W] and
    through to_planes / from_planes on [B,C,P,H,W].  (On the CPU; tests/test_conv2d_geometry.py runs it without a GPU as well.)"""
    B, Ci, Co, H, W = shape
    x, w = seeded("c2.rs.x", B, Ci, H, W).double(), seeded("c2.rs.w", Co, Ci, 3, 3).double()
    G = seeded("c2.rs.G", B, Co, H, W).double()
    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv2d(xs, ws, None, 1, 1)
    y.backward(G)
    for got, ref in ((wino2_fwd(x, w), y.detach()), (wino2_dgrad(G, w), xs.grad), (wino2_wgrad(x, G), ws.grad)):
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    x5 = seeded("c2.rs.x5", B, Ci, 3, H, W).double()
    assert torch.equal(from_planes(to_planes(x5), B), x5)
    y5 = torch.stack([F.conv2d(x5[:, :, p], w, None, 1, 1) for p in range(3)], 2)
    got = from_planes(wino2_fwd(to_planes(x5), w), B)
    assert got.shape == y5.shape and float((got - y5).abs().max()) <= 1e-12 * float(y5.abs().max())


CHAIN_SHAPES = [((3, 3), 1, 1, None), ((3, 3), 1, 2, None), ((3, 3), 1, 4, None), ((3, 3), 2, 1, None), ((3, 5), 1, 1, None),
                ((3, 5), 1, 1, "Q"), ((1, 1), 1, 1, None), ((1, 1), 2, 1, None)]


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=str)
def test_chain2d_restatement_is_the_convolution(shape):
    """chain_conv2d -- forward, and the data gradient as ops forms it (flip-transposed weight, padding (K - 1) * dil - pad; zero
    insertion after the 1x1 at stride 2) -- in fp64 equals F.conv2d and its autograd in fp64 to 1e-12 of scale (on the CPU)."""
    k, stride, dil, cls = shape
    c = Case("conv", 2, 6, 5, 9, 11, k, stride, dil, cls=cls)
    pt, pl, Ho, Wo = geometry(c)
    x, w = seeded("c2.ch.x", 2, 6, 9, 11).double(), seeded("c2.ch.w", 5, 6, *k).double()
    xs = x.clone().requires_grad_()
    y = conv_ref(xs, w, stride, dil, pt, pl, Ho, Wo)
    assert y.shape[-2:] == (Ho, Wo)
    G = seeded("c2.ch.G", *y.shape).double()
    y.backward(G)
    pairs = [(chain_conv2d(x, w, stride, dil, pt, pl, Ho, Wo, 4), y.detach())]
    if stride == 1:
        pairs.append((chain_conv2d(G, flip_t(w), 1, dil, (k[0] - 1) * dil - pt, (k[1] - 1) * dil - pl, 9, 11, 4), xs.grad))
    elif k == (1, 1):
        pairs.append((zero_insert(chain_conv2d(G, flip_t(w), 1, 1, 0, 0, Ho, Wo, 8), 9, 11), xs.grad))
    for got, ref in pairs:
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv2d_fp64(ecm, name):
    """Every quantity of one case of the table on every kernel it dispatches to: the fp64 bound, bit-identical repeats."""
    _run_case(ecm, name)
