"""The 3-D convolution kernels against fp64, on every tile path of csrc/conv3d.hip, conv_wino.hip, conv3d_wgrad.hip, deconv3d.hip
and conv3d_c1.hip.

Which kernel instantiation runs, how many tiles a persistent worker walks and whether a tile is ragged is decided silently by the
shape (`ecm_conv3d_k3_fwd`'s `small` threshold, `wgrad_workers`, `c1_workers`, `_wino_ok`, `_is_c1`).  The case table below names,
for every path class and every edge inside a path, a shape that reaches it; the host-side dispatch is restated here in Python so
that the mapping is asserted (tests/test_conv3d_geometry.py pins the constants to the sources and asserts `missing_classes() == []`
on the CPU) instead of assumed.  All operations are reached through ecm_amd.ops as the model reaches them (ops.conv3d_k3,
ops.deconv3d_k3s2 and their autograd); two weight-gradient schedules go through ops._wgrad alone: six channel tiles at stride 2, which no
layer shape the stride-2 kernels accept (at most 64 channels either way) can produce, and sixteen channel tiles (128 -> 128).

Yardstick (the one of test_hip_numerics.py and test_hip_groupnorm_fp64.py).  Reference: F.conv3d / F.conv_transpose3d and autograd
in fp64 on the CPU; operands from oracle.weights.seeded under a name per case, weights He-scaled.  Unit: the reference's OWN fp32
error, e32(q) = max |q32 - q64| over independent fp32 evaluations of the same expression: torch's on the CPU, torch's on the device,
and -- for the quantities a Winograd kernel produced only -- a plain-torch fp32 restatement of F(2x2,3x3) written below (V = B^T d B,
U = G g G^T, a per-frequency contraction over (kd, ci), Y = A^T M A; the weight-gradient form likewise), because the transforms have
an fp32 error of their own.  `test_winograd_restatement_is_the_convolution` shows that restatement equal to the reference in fp64.
For what conv3d_k3_mfma produced (direct forward, the flip-transposed stride-1 data gradient, the stride-2 data gradient of
ops.deconv3d_k3s2) a further candidate is the operation in that kernel's own summation order, `chain_conv`: the kernel is one fmaf
chain per output over (chunk of CIC channels, tap, channel), 27 * Ci terms one after another, where torch's convolutions sum in
blocks.  A chain of 864 terms (32 channels) is 5.4 x further from fp64 than torch on d_s1_t1_small_c2's data gradient (1.15e-05
against 2.1e-06; the same figure from an fp32 fma chain evaluated on the CPU, bit for bit the kernel's), which K = 4 does not
contain; K stays 4 and the unit takes the plain-torch fp32 chain (mul, then add) as the issue's summation-order rule prescribes.
`test_chain_restatement_is_the_convolution` shows it equal to the reference in fp64.  No other path has that candidate.
A kernel passes when  max|q_hip - q64| <= K * e32(q) + FLOOR * max|q64|  with K = 4, FLOOR = 2e-7, for q in {y, gx, gw}.  With
fork=True, gx must meet the same bound against the fp64 value of dgrad + gskip.

Every case runs twice on fresh operands and y, gx, gw must reproduce bit for bit (the kernels claim fixed-order reductions).
Operands differ between cases and all outputs of a case stay alive until it ends, so an element a kernel failed to write cannot
inherit the right value from recycled memory.

Each test prints `C3RATIO <path> <quantity> <ratio>` with ratio = |q_hip - q64| / (K * e32 + floor); DESIGN.md section 4 holds the
worst ratio per path and quantity as measured on the MI355X."""
import collections
import contextlib

import pytest
import torch
import torch.nn.functional as F

from oracle.weights import seeded

pytestmark = pytest.mark.gpu

K, FLOOR = 4.0, 2e-7            # test_hip_numerics.py: 4 x torch's own fp32 error + one fp32 ulp of the output scale
DEV = "cuda"


def cdiv(a, b):
    return -(-a // b)


# ---- the host-side dispatch, restated (tests/test_conv3d_geometry.py pins every constant to its source) -------------------------
TW = 32                         # fp32_conv_stage.h: output columns per tile (conv3d.hip, deconv3d.hip)
TWV, CT = 16, 32                # conv3d_wgrad.hip: output voxels per tile row, channel tile
SMALL_BLOCKS = 384              # ecm_conv3d_k3_fwd: fewer 2x8x32 blocks than this -> the 1x4x32 tile
# (stride, Co > 32, small) -> launch_conv<CO_TILES, STRIDE, TD, TH, CIC>
FWD_INST = {(1, False, True): (1, 1, 1, 4, 4), (1, False, False): (1, 1, 4, 8, 4), (1, True, True): (2, 1, 1, 4, 4),
            (1, True, False): (2, 1, 2, 8, 4), (2, False, True): (1, 2, 1, 4, 2), (2, False, False): (1, 2, 2, 8, 2),
            (2, True, True): (2, 2, 1, 4, 2), (2, True, False): (2, 2, 2, 8, 2)}
WGRAD_WORKERS, WGRAD_OCC3D = 256, 1
# launch_wgrad<STRIDE, TD, TH, KD> / launch_wgrad_wino<TD, TH, KD>
WGRAD_INST = {"s1": (1, 2, 8, 3), "s2": (2, 1, 4, 3), "wino": (2, 8, 3)}
WINO_CIC3 = 2
WINO_INST = (3, 2, 1, WINO_CIC3)        # launch_wino<KD, TD, TR, CIC>
WINO_BLOCK = 32                         # consecutive 2x2 tiles per workgroup (x TR)
DECONV_TD, DECONV_TH, DECONV_CIC = 1, 4, 4
DECONV_INST = {False: (1, DECONV_CIC), True: (2, DECONV_CIC)}       # launch_deconv<CO_TILES, CIC>
VT_W, VT_H, VT_D = 32, 16, 8            # conv3d_c1_fwd_v
DTH, DTW = 8, 128                       # conv3d_c1_dgrad
GTD, GTH, GTW = 2, 8, 32                # conv3d_c1_wgrad
C1_WORKERS = 512


def out_dims(dims, stride):
    return tuple((d - 1) // stride + 1 for d in dims)


def is_c1(Co, Ci, stride):
    """ops._is_c1"""
    return Co == 1 and stride == 1 and Ci <= 32 and Ci % 8 == 0


def wino_ok(dims, winograd=True):
    """ops._wino_ok"""
    return winograd and dims[2] >= 2 and dims[0] * dims[1] * dims[2] * 128 <= 0x80000000


def direct_fwd(B, Ci, Co, dims, stride):
    """ecm_conv3d_k3_fwd on x [B, Ci, *dims]: the instantiation, its grid, the number of input-channel chunks, raggedness."""
    assert Ci % 4 == 0 and 1 <= Co <= 64 and stride in (1, 2), "ECM_EUNSUP"
    Do, Ho, Wo = out_dims(dims, stride)
    small = B * cdiv(Do, 2) * cdiv(Ho, 8) * cdiv(Wo, TW) < SMALL_BLOCKS
    inst = FWD_INST[(stride, Co > 32, small)]
    _, _, TD, TH, CIC = inst
    return dict(inst=inst, small=small, nblk=B * cdiv(Do, TD) * cdiv(Ho, TH) * cdiv(Wo, TW), chunks=Ci // CIC,
                ragged=(Do % TD != 0, Ho % TH != 0, Wo % TW != 0), Co=Co)


def worker_runs(P, ntiles):
    """Tiles walked by each of the P persistent workers of conv3d_wgrad_mfma: one contiguous run per XCD when P % 8 == 0
    (lengths q or q + 1, the workers of an XCD striding through it), else tile0 = worker, step = P."""
    runs = []
    for p in range(P):
        if P % 8 == 0:
            xcd, q, rr = p & 7, ntiles >> 3, ntiles & 7
            start = xcd * q + min(xcd, rr)
            runs.append(len(range(start + (p >> 3), start + q + (1 if xcd < rr else 0), P >> 3)))
        else:
            runs.append(len(range(p, ntiles, P)))
    return runs


def wgrad_geom(kind, B, Ci, Co, dims):
    """launch_wgrad<1,2,8,3> ("s1"), <2,1,4,3> ("s2") or launch_wgrad_wino<2,8,3> ("wino") for x [B, Ci, *dims], gw [Co, Ci, 27]."""
    inst = WGRAD_INST[kind]
    stride, TD, TH = (1,) + inst[:2] if kind == "wino" else inst[:3]
    o = out_dims(dims, stride)
    ntiles = B * cdiv(o[0], TD) * cdiv(o[1], TH) * cdiv(o[2], TWV)
    ytiles = cdiv(Ci, CT) * cdiv(Co, CT)
    P = min(max(1, WGRAD_WORKERS * WGRAD_OCC3D // ytiles), ntiles)
    return dict(kind=kind, inst=inst, ntiles=ntiles, ytiles=ytiles, P=P, runs=worker_runs(P, ntiles), out=o,
                ragged=tuple(n % t != 0 for n, t in zip(o, (TD, TH, TWV)) if t > 1), ragged_ch=(Ci % CT != 0, Co % CT != 0))


def wino_geom(B, Ci, Co, dims):
    """launch_wino<3,2,1,WINO_CIC3> for x [B, Ci, *dims] -> Co channels."""
    KD, TD, TR, CIC = WINO_INST
    D, H, W = dims
    tiles_wt = (W + 1) // 2
    ntile = ((H + 1) // 2) * tiles_wt
    return dict(tiles_wt=tiles_wt, ntile=ntile, tblocks=cdiv(ntile, WINO_BLOCK * TR), nchunks=cdiv(Ci, CIC), groups=cdiv(Co, 32),
                Ci=Ci, Co=Co, dims=dims)


def deconv_geom(B, Ci, Co, in_dims, o_dims):
    """ecm_deconv3d_k3s2_fwd on x [B, Ci, *in_dims] -> [B, Co, *o_dims] (each extent 2n or 2n - 1)."""
    assert Ci % 4 == 0 and 1 <= Co <= 64 and all(2 * n - 1 <= o <= 2 * n for n, o in zip(in_dims, o_dims)), "ECM_EUNSUP"
    D, H, W = in_dims
    return dict(inst=DECONV_INST[Co > 32], nblk=B * cdiv(D, DECONV_TD) * cdiv(H, DECONV_TH) * cdiv(W, TW),
                parity=tuple(o % 2 for o in o_dims), ragged=(H % DECONV_TH != 0, W % TW != 0), chunks=Ci // DECONV_CIC)


def c1_geom(B, Ci, dims):
    D, H, W = dims
    nt = B * cdiv(D, GTD) * cdiv(H, GTH) * cdiv(W, GTW)
    P = min(nt, C1_WORKERS)
    return dict(fwd_ragged=(D % VT_D != 0, H % VT_H != 0, W % VT_W != 0), fwd_blocks=B * cdiv(D, VT_D) * cdiv(H, VT_H) * cdiv(W, VT_W),
                dgrad_ragged=(H % DTH != 0, W % DTW != 0), wgrad_tiles=nt, wgrad_P=P, wgrad_runs=[len(range(p, nt, P)) for p in range(P)])


# ---- the case table ------------------------------------------------------------------------------------------------------------
# op: "conv" = ops.conv3d_k3(x, w, stride) fwd + bwd; "deconv" = ops.deconv3d_k3s2 fwd + bwd; "wgrad" = ops._wgrad alone.
# wino: the value of ops.WINOGRAD for the case; fork: the fork=True addend; frozen: forward under ops.frozen_weights(), so that no
# data-gradient layout is packed in forward and the backward packs afresh (ecm_conv_wino_pack_weight, flip_transpose = 1).
Case = collections.namedtuple("Case", "op B Ci Co dims stride wino fork frozen", defaults=(1, True, False, False))
_BIG = (49, 9, 33)              # 4 x 25 x 2 x 2 = 400 blocks of 2x8x32: ragged in D for TD = 4 and TD = 2, ragged in H and W

DIRECT = {
    # ecm_conv3d_k3_fwd, the four 1x4x32 instantiations; Ci / CIC = 1, 2, 3 (stride 1) and 2, 4, 6 (stride 2; Ci % 4 == 0)
    "d_s1_t1_small_c1": Case("conv", 1, 4, 8, (3, 5, 9), 1, False),               # 6 blocks: fewer than the 8 XCDs
    "d_s1_t1_small_c2": Case("conv", 1, 8, 32, (5, 7, 37), 1, False),             # 20 blocks: unequal runs per XCD
    "d_s1_t1_small_c3": Case("conv", 2, 12, 32, (3, 4, 32), 1, False),            # nothing ragged
    "d_s1_t2_small": Case("conv", 1, 12, 40, (3, 5, 35), 1, False),
    "d_s1_t2_small_co64": Case("conv", 2, 8, 64, (2, 6, 33), 1, False),
    "d_s2_t1_small_c2": Case("conv", 1, 4, 8, (5, 7, 9), 2, False),               # every extent odd: data gradient 2n - 1
    "d_s2_t1_small_c4": Case("conv", 1, 8, 32, (9, 14, 70), 2, False),            # 20 blocks; D odd, H and W even
    "d_s2_t2_small": Case("conv", 2, 12, 40, (6, 10, 70), 2, False),              # every extent even: data gradient 2n
    "d_s2_t2_small_co64": Case("conv", 1, 32, 64, (8, 16, 24), 2, False),
    "d_s2_dgrad_t2": Case("conv", 1, 64, 8, (5, 8, 67), 2, False),                # data gradient: deconv<2,4>, D and W odd, H even
    # the four large-tile instantiations (the production ones), forward
    "d_s1_t1_large_co8": Case("conv", 4, 12, 8, _BIG, 1, False),
    "d_s1_t2_large_co40": Case("conv", 4, 12, 40, _BIG, 1, False),
    "d_s2_t1_large": Case("conv", 4, 12, 32, (97, 17, 65), 2, False),
    "d_s2_t2_large": Case("conv", 4, 12, 64, (98, 18, 66), 2, False),
    # ... and as the flip-transposed stride-1 data gradient, where Ci plays Co
    "d_s1_large_64_32": Case("conv", 4, 64, 32, _BIG, 1, False),
    "d_s1_large_32_64": Case("conv", 4, 32, 64, _BIG, 1, False),
}
WINO = {
    # conv_wino<3,2,1,2> forward and data gradient; both weight-gradient forms run on every case
    "w_ci2_rows_wrap": Case("conv", 1, 2, 8, (3, 5, 6)),                  # one chunk; 9 tiles of 3 per row: a block spans rows, ends ragged
    "w_ci4_w2": Case("conv", 1, 4, 4, (2, 3, 2)),                         # two chunks; W = 2
    "w_ci6_w3_co40": Case("conv", 1, 6, 40, (2, 5, 3)),                   # three chunks; W = 3; second channel group of 8
    "w_ci3_odd": Case("conv", 1, 3, 64, (3, 4, 7)),                       # odd Ci: half a chunk of padding
    "w_ci8_w3": Case("conv", 1, 8, 8, (2, 5, 3)),
    "w_w65": Case("conv", 1, 16, 16, (2, 3, 65)), "w_w66": Case("conv", 1, 32, 32, (2, 4, 66)),
    "w_w127": Case("conv", 1, 16, 16, (1, 3, 127)), "w_w128": Case("conv", 1, 16, 16, (2, 2, 128)),
    "w_w129": Case("conv", 1, 8, 8, (1, 4, 129)),
    "w_w130_co40": Case("conv", 1, 32, 40, (2, 4, 130)),                  # 65 tiles per row
    "w_odd_all": Case("conv", 2, 32, 32, (5, 7, 35)),
    "w_64_64": Case("conv", 1, 64, 64, (3, 9, 33)),
    "w_fork_odd": Case("conv", 1, 32, 32, (3, 7, 35), fork=True),
    "w_fork_co40": Case("conv", 1, 8, 40, (2, 5, 67), fork=True),
    "w_fresh_pack": Case("conv", 1, 32, 64, (3, 6, 34), frozen=True),
}
WGRAD = {
    # persistent schedules of conv3d_wgrad_mfma: P < ntiles
    "g_s1_xcd": Case("conv", 2, 64, 64, (9, 17, 33)),                     # wino + <1,2,8,3>: P = 64, 90 tiles: XCD runs of 12 and 11
    "g_s1_strided": Case("conv", 2, 40, 72, (5, 10, 50)),                 # wino + <1,2,8,3>: P = 42, 48 tiles; channel tiles of 8
    "g_s2_xcd": Case("conv", 3, 64, 64, (9, 17, 35), 2, False),           # <2,1,4,3>: P = 64, 90 tiles
    "g_s2_strided": Case("wgrad", 2, 40, 72, (9, 17, 35), 2, False),      # <2,1,4,3>: P = 42, 60 tiles
    "g_c128": Case("wgrad", 1, 128, 128, (5, 9, 33)),                     # wino + <1,2,8,3>: 16 channel tiles, P = 16, 18 tiles
}
DECONV = {
    # ops.deconv3d_k3s2: deconv3d.hip forward (all 2n), stride-2 direct data gradient, role-exchanged weight gradient
    "t_64_64": Case("deconv", 1, 64, 64, (2, 4, 6)),
    "t_64_32_ragged": Case("deconv", 2, 64, 32, (3, 5, 35)),
    "t_8_40": Case("deconv", 1, 8, 40, (3, 5, 33)),
    "t_persistent": Case("deconv", 3, 64, 64, (5, 9, 18)),                # role-exchanged <2,1,4,3>: P = 64, 90 tiles
    "t_4_32_one_chunk": Case("deconv", 1, 4, 32, (2, 5, 33)),             # Ci = CIC: the chunk loop without a prefetch; H, W ragged
}
C1 = {
    # the 32 -> 1 layer: conv3d_c1_fwd_v<false>, conv3d_c1_dgrad, conv3d_c1_wgrad
    "c_ci8": Case("conv", 1, 8, 1, (9, 17, 33)), "c_ci16": Case("conv", 1, 16, 1, (5, 7, 33)),
    "c_ci24": Case("conv", 1, 24, 1, (10, 18, 40)), "c_ci32": Case("conv", 2, 32, 1, (20, 14, 70)),
    "c_w127": Case("conv", 1, 8, 1, (2, 5, 127)), "c_w128": Case("conv", 1, 16, 1, (2, 9, 128)), "c_w129": Case("conv", 1, 8, 1, (3, 6, 129)),
    "c_persistent": Case("conv", 6, 8, 1, (33, 17, 33)),                  # 612 tiles of 2x8x32 on 512 workers: 100 of them walk two
}
CASES = {**DIRECT, **WINO, **WGRAD, **DECONV, **C1}


def launches(c):
    """Every kernel launch a case makes, as (role, geometry): what ops.Conv3dK3 / ops.Deconv3dK3S2 / ops._wgrad dispatch to."""
    o = out_dims(c.dims, c.stride)
    if c.op == "wgrad":
        kinds = ["wino", "s1"] if c.stride == 1 and wino_ok(c.dims, c.wino) else ["s1" if c.stride == 1 else "s2"]
        return [("gw", "wgrad", wgrad_geom(k, c.B, c.Ci, c.Co, c.dims)) for k in kinds]
    if c.op == "deconv":
        up = tuple(2 * d for d in c.dims)
        return [("y", "deconv", deconv_geom(c.B, c.Ci, c.Co, c.dims, up)),
                ("gx", "direct", direct_fwd(c.B, c.Co, c.Ci, up, 2)),
                ("gw", "wgrad", dict(wgrad_geom("s2", c.B, c.Co, c.Ci, up), exchanged=True))]
    if is_c1(c.Co, c.Ci, c.stride):
        g = c1_geom(c.B, c.Ci, c.dims)
        return [("y", "c1", g), ("gx", "c1", g), ("gw", "c1", g)]
    if c.stride == 1 and wino_ok(c.dims, c.wino):
        return [("y", "wino", wino_geom(c.B, c.Ci, c.Co, c.dims)),
                ("gx", "wino", dict(wino_geom(c.B, c.Co, c.Ci, c.dims), add=c.fork, fresh=c.frozen)),
                ("gw", "wgrad", wgrad_geom("wino", c.B, c.Ci, c.Co, c.dims)), ("gw", "wgrad", wgrad_geom("s1", c.B, c.Ci, c.Co, c.dims))]
    out = [("y", "direct", direct_fwd(c.B, c.Ci, c.Co, c.dims, c.stride))]
    if c.stride == 1:
        out.append(("gx", "direct", dict(direct_fwd(c.B, c.Co, c.Ci, c.dims, 1), dgrad=True)))
    else:
        out.append(("gx", "deconv", deconv_geom(c.B, c.Co, c.Ci, o, c.dims)))
    out.append(("gw", "wgrad", wgrad_geom("s1" if c.stride == 1 else "s2", c.B, c.Ci, c.Co, c.dims)))
    return out


def path_name(q, fam, g):
    if fam == "c1":
        return {"y": "c1_fwd_v", "gx": "c1_dgrad", "gw": "c1_wgrad"}[q]
    if fam == "direct":
        return "conv<%d,%d,%d,%d,%d>" % g["inst"] + (":dgrad" if g.get("dgrad") else "")
    if fam == "deconv":
        return "deconv<%d,%d>" % g["inst"]
    if fam == "wino":
        return "wino<%d,%d,%d,%d>" % WINO_INST + ("+add" if g.get("add") else "")
    if fam == "wgrad":
        return ("wgrad_wino<%d,%d,%d>" if g["kind"] == "wino" else "wgrad<%d,%d,%d,%d>") % g["inst"] + (":exchanged" if g.get("exchanged") else "")
    raise KeyError(fam)


def missing_classes():
    """The path classes (module docstring, case table) that NO case reaches under the restated dispatch."""
    L = [(name, q, fam, g) for name, c in CASES.items() for q, fam, g in launches(c)]
    direct = [g for _, _, fam, g in L if fam == "direct"]
    wino = [(q, g) for _, q, fam, g in L if fam == "wino"]
    wg = [g for _, _, fam, g in L if fam == "wgrad"]
    dec = [(q, g) for _, q, fam, g in L if fam == "deconv"]
    c1 = [g for _, q, fam, g in L if fam == "c1" and q == "y"]
    want = {}
    for inst in FWD_INST.values():
        want["direct forward %s" % (inst,)] = any(g["inst"] == inst and not g.get("dgrad") for g in direct)
    for inst in (FWD_INST[(1, False, False)], FWD_INST[(1, True, False)]):
        want["direct forward %s ragged in D, H and W" % (inst,)] = any(g["inst"] == inst and all(g["ragged"]) for g in direct)
        want["direct stride-1 data gradient on %s" % (inst,)] = any(g["inst"] == inst and g.get("dgrad") for g in direct)
    for inst in (FWD_INST[(2, False, False)], FWD_INST[(2, True, False)]):
        want["direct forward %s with a ragged output grid" % (inst,)] = any(g["inst"] == inst and any(g["ragged"]) for g in direct)
    for n in (1, 2, 3):
        want["direct %s: %d chunk(s) of CIC" % (FWD_INST[(1, False, True)], n)] = any(
            g["inst"] == FWD_INST[(1, False, True)] and (g["chunks"] == n if n < 3 else g["chunks"] >= 3) for g in direct)
    for n in (2, 3):            # Ci % 4 == 0 and CIC = 2: never a single chunk
        want["direct %s: %s chunks of CIC" % (FWD_INST[(2, False, True)], n if n < 3 else ">= 3")] = any(
            g["inst"] == FWD_INST[(2, False, True)] and (g["chunks"] == n if n < 3 else g["chunks"] >= 3) for g in direct)
    for co in (8, 32, 40, 64):
        want["direct forward Co = %d" % co] = any(g["Co"] == co and not g.get("dgrad") for g in direct)
        want["winograd forward Co = %d" % co] = any(q == "y" and g["Co"] == co for q, g in wino)
    want["direct: nblk % 8 != 0 (unequal XCD runs)"] = any(g["nblk"] > 8 and g["nblk"] % 8 for g in direct)
    want["direct: nblk < 8"] = any(g["nblk"] < 8 for g in direct)
    # Winograd forward / data gradient
    wf = [g for q, g in wino if q == "y"]
    for i, n in enumerate("DHW"):
        want["winograd: %s odd" % n] = any(g["dims"][i] % 2 for g in wf)
    for w in (2, 3, 65, 66, 127, 128, 129):
        want["winograd: W = %d" % w] = any(g["dims"][2] == w for g in wf)
    want["winograd: a block spans several rows and ends ragged"] = any(g["tiles_wt"] < WINO_BLOCK and g["ntile"] % WINO_BLOCK
                                                                       and g["ntile"] > g["tiles_wt"] for g in wf)
    want["winograd: more than 32 tiles per row, no multiple of 32"] = any(g["tiles_wt"] > WINO_BLOCK and g["tiles_wt"] % WINO_BLOCK for g in wf)
    for ci in (2, 4, 6, 32, 64):
        want["winograd forward Ci = %d" % ci] = any(g["Ci"] == ci for g in wf)
    for n in (1, 2, 3):
        want["winograd: %d chunk(s)" % n] = any(g["nchunks"] == n for g in wf)
    want["winograd: odd Ci"] = any(g["Ci"] % 2 for g in wf)
    want["winograd: second channel group not full"] = any(g["groups"] == 2 and g["Co"] % 32 for g in wf)
    wd = [g for q, g in wino if q == "gx"]
    want["winograd data gradient + addend, H and W odd"] = any(g["add"] and g["dims"][1] % 2 and g["dims"][2] % 2 for g in wd)
    want["winograd data gradient, layout packed in forward"] = any(not g["fresh"] for g in wd)
    want["winograd data gradient, layout packed afresh"] = any(g["fresh"] for g in wd)
    # weight gradients
    for kind in WGRAD_INST:
        k = [g for g in wg if g["kind"] == kind]
        lab = "wgrad %s %s: " % (kind, WGRAD_INST[kind])          # (ragged: against every tile extent above 1)
        want[lab + "P == ntiles"] = any(g["P"] == g["ntiles"] for g in k)
        want[lab + "P < ntiles, P % 8 == 0, ntiles % 8 != 0"] = any(g["P"] < g["ntiles"] and g["P"] % 8 == 0 and g["ntiles"] % 8 for g in k)
        want[lab + "P < ntiles, P % 8 != 0"] = any(g["P"] < g["ntiles"] and g["P"] % 8 for g in k)
        want[lab + "neighbouring workers walk n + 1 and n >= 1 tiles"] = any(
            any(a == b + 1 and b >= 1 for a, b in zip(g["runs"], g["runs"][1:])) for g in k)
        want[lab + "ragged in D, H and W"] = any(all(g["ragged"]) for g in k)
        want[lab + "ragged channel tiles"] = any(all(g["ragged_ch"]) for g in k)
    kw = [g for g in wg if g["kind"] == "wino"]
    want["wgrad wino: H odd"] = any(g["out"][1] % 2 for g in kw)
    for r in (1, 2, 3):
        want["wgrad wino: W %% 4 = %d" % r] = any(g["out"][2] % 4 == r for g in kw)
    want["wgrad s2: role-exchanged (Deconv3dK3S2.backward)"] = any(g.get("exchanged") for g in wg)
    want["wgrad s2: role-exchanged, P < ntiles"] = any(g.get("exchanged") and g["P"] < g["ntiles"] for g in wg)
    # deconv3d.hip
    for two in (False, True):
        want["deconv %s" % (DECONV_INST[two],)] = any(g["inst"] == DECONV_INST[two] for _, g in dec)
    want["deconv: every output extent even"] = any(g["parity"] == (0, 0, 0) for q, g in dec if q == "gx")
    want["deconv: every output extent odd"] = any(g["parity"] == (1, 1, 1) for q, g in dec if q == "gx")
    for i, n in enumerate("DHW"):
        for par in (0, 1):
            want["deconv: %s output %s" % (n, "2n - 1" if par else "2n")] = any(g["parity"][i] == par for _, g in dec)
    want["deconv: ragged against 4 x 32"] = any(all(g["ragged"]) for _, g in dec)
    want["deconv forward (ops.deconv3d_k3s2)"] = any(q == "y" for q, _ in dec)
    for n in (1, 2, 3):         # the regimes of the shared chunk loop (fp32_conv_stage.h): no prefetch, one, a prefetch of a prefetch
        want["deconv: %s chunk(s) of CIC" % (n if n < 3 else ">= 3")] = any(g["chunks"] == n if n < 3 else g["chunks"] >= 3 for _, g in dec)
    # 32 -> 1
    for ci in (8, 16, 24, 32):
        want["c1: Ci = %d, forward ragged" % ci] = any(c.Ci == ci and is_c1(c.Co, c.Ci, c.stride) and any(c1_geom(c.B, c.Ci, c.dims)["fwd_ragged"])
                                                       for c in CASES.values() if c.op == "conv")
    for w in (127, 128, 129):
        want["c1 data gradient: W = %d, H %% 8 != 0" % w] = any(c.dims[2] == w and c.dims[1] % DTH and is_c1(c.Co, c.Ci, c.stride)
                                                                for c in CASES.values())
    want["c1 forward: ragged in D, H and W"] = any(all(g["fwd_ragged"]) for g in c1)
    want["c1 weight gradient: one tile per worker"] = any(g["wgrad_tiles"] <= C1_WORKERS for g in c1)
    want["c1 weight gradient: persistent, with a remainder"] = any(g["wgrad_tiles"] > C1_WORKERS and g["wgrad_tiles"] % C1_WORKERS for g in c1)
    return sorted(k for k, ok in want.items() if not ok)


# ---- F(2x2,3x3) in plain torch, in the dtype of its operands ---------------------------------------------------------------------
_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def _mats(t):
    return [torch.tensor(m, dtype=t.dtype, device=t.device) for m in (_BT, _G, _AT)]


def _wino_v(x):
    """V = B^T d B of every 4x4 patch (2x2 output tiles, zero padding): [B, Ci, D, th, tw, 4, 4, kd]"""
    H, W = x.shape[-2:]
    d = F.pad(x, (1, 1 + W % 2, 1, 1 + H % 2, 1, 1)).unfold(3, 4, 2).unfold(4, 4, 2)
    BT = _mats(x)[0]
    return (BT @ d @ BT.T).unfold(2, 3, 1)


def wino_fwd(x, w):
    """conv3d(x, w, stride 1, pad 1) as the Winograd kernel forms it: H, W by F(2x2,3x3), depth taps and channels contracted
    per frequency."""
    _, G, AT = _mats(x)
    B, _, D, H, W = x.shape
    M = torch.einsum("ockij,bcdtuijk->bodtuij", G @ w @ G.T, _wino_v(x))
    Y = AT @ M @ AT.T
    th, tw = Y.shape[3:5]
    return Y.permute(0, 1, 2, 3, 5, 4, 6).reshape(B, -1, D, 2 * th, 2 * tw)[..., :H, :W]


def wino_dgrad(gy, w):
    return wino_fwd(gy, w.flip(2, 3, 4).transpose(0, 1))


def wino_wgrad(x, gy):
    """gw = G^T [ sum over tiles (A gy A^T) . (B^T d B) ] G"""
    _, G, AT = _mats(x)
    H, W = gy.shape[-2:]
    gt = F.pad(gy, (0, W % 2, 0, H % 2)).unfold(3, 2, 2).unfold(4, 2, 2)
    gU = torch.einsum("bodtuij,bcdtuijk->ockij", AT.T @ gt @ AT, _wino_v(x))
    return G.T @ gU @ G


# ---- the direct kernel's own summation order in plain torch ---------------------------------------------------------------------
def chain_conv(x, w, stride, cic):
    """conv3d(x, w, stride, pad 1) as conv3d_k3_mfma sums it: ONE chain per output element, acc <- acc + w * x one term after
    another over (chunk of `cic` input channels, tap, channel of the chunk), in the dtype of the operands."""
    B, Ci = x.shape[:2]
    o = out_dims(x.shape[2:], stride)
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    acc = x.new_zeros(B, w.shape[0], *o)
    for c0 in range(0, Ci, cic):
        for kd, kh, kw in ((a, b, c) for a in range(3) for b in range(3) for c in range(3)):
            for c in range(c0, min(c0 + cic, Ci)):
                win = xp[:, c:c + 1, kd:kd + (o[0] - 1) * stride + 1:stride, kh:kh + (o[1] - 1) * stride + 1:stride,
                         kw:kw + (o[2] - 1) * stride + 1:stride]
                acc = acc + w[:, c, kd, kh, kw].view(1, -1, 1, 1, 1) * win
    return acc


def chain_dgrad(gy, w, cic):
    """the stride-1 data gradient as ops runs it: the same kernel on the flip-transposed weight"""
    return chain_conv(gy, w.flip(2, 3, 4).transpose(0, 1), 1, cic)


# ---- fixtures and helpers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def _operands(name, c):
    """x, w, G (the gradient of y), Gs (the gradient arriving at the forked input, or None)"""
    o = tuple(2 * d for d in c.dims) if c.op == "deconv" else out_dims(c.dims, c.stride)
    x = seeded("c3." + name + ".x", c.B, c.Ci, *c.dims)
    wshape = (c.Ci, c.Co) if c.op == "deconv" else (c.Co, c.Ci)
    w = seeded("c3." + name + ".w", *wshape, 3, 3, 3) * (2.0 / (27 * c.Ci)) ** 0.5
    G = seeded("c3." + name + ".G", c.B, c.Co, *o)
    Gs = seeded("c3." + name + ".Gs", *x.shape) if c.fork else None
    return x, w, G, Gs


def _torch(c, x, w, G, Gs, dtype, device):
    """The expression in `dtype` on `device` through torch's own convolution and autograd."""
    cv = lambda t: t.detach().to(device=device, dtype=dtype, copy=True)                 # noqa: E731
    xs, ws = cv(x).requires_grad_(c.op != "wgrad"), cv(w).requires_grad_()
    y = F.conv_transpose3d(xs, ws, None, 2, 1, 1) if c.op == "deconv" else F.conv3d(xs, ws, None, c.stride, 1)
    y.backward(cv(G))
    if c.op == "wgrad":
        return {"gw": ws.grad}
    return {"y": y.detach(), "gx": xs.grad if Gs is None else xs.grad + cv(Gs), "gw": ws.grad}


def _wino32(c, x, w, G, Gs):
    """The fp32 Winograd restatement on the device, for the quantities of a stride-1 convolution."""
    x, w, G = x.to(DEV), w.to(DEV), G.to(DEV)
    gx = wino_dgrad(G, w)
    return {"y": wino_fwd(x, w), "gx": gx if Gs is None else gx + Gs.to(DEV), "gw": wino_wgrad(x, G)}


def _chain32(c, L, x, w, G, Gs):
    """The fp32 chain restatement on the device, for the quantities conv3d_k3_mfma produced (its CIC from the restated dispatch)."""
    out = {}
    for q, fam, g in L:
        if fam != "direct":
            continue
        cic = g["inst"][4]
        if q == "y":
            out["y"] = chain_conv(x.to(DEV), w.to(DEV), c.stride, cic)
        elif c.op == "deconv":                  # Deconv3dK3S2.backward: the stride-2 convolution of G by the same weight
            out["gx"] = chain_conv(G.to(DEV), w.to(DEV), 2, cic)
        else:
            gx = chain_dgrad(G.to(DEV), w.to(DEV), cic)
            out["gx"] = gx if Gs is None else gx + Gs.to(DEV)
    return out


@contextlib.contextmanager
def switches(ecm, winograd, winograd_wgrad):
    prev = ecm.ops.WINOGRAD, ecm.ops.WINOGRAD_WGRAD
    ecm.ops.WINOGRAD, ecm.ops.WINOGRAD_WGRAD = winograd, winograd_wgrad
    try:
        yield
    finally:
        ecm.ops.WINOGRAD, ecm.ops.WINOGRAD_WGRAD = prev


def _hip(ecm, c, x, w, G, Gs):
    """The operation through ecm_amd.ops on fresh copies of the operands."""
    ops = ecm.ops
    xg, wg, Gd = x.to(DEV).requires_grad_(c.op != "wgrad"), w.to(DEV).requires_grad_(), G.to(DEV)
    if c.op == "wgrad":
        return {"gw": ops._wgrad(xg, Gd, c.Co, c.Ci, c.stride)}
    with (ops.frozen_weights() if c.frozen else contextlib.nullcontext()):
        if c.op == "deconv":
            y = ops.deconv3d_k3s2(xg, wg)
        elif c.fork:
            y, xa = ops.conv3d_k3(xg, wg, c.stride, fork=True)
            assert xa.data_ptr() == xg.data_ptr()
        else:
            y = ops.conv3d_k3(xg, wg, c.stride)
    if c.fork:
        torch.autograd.backward([y, xa], [Gd, Gs.to(DEV)])
    else:
        y.backward(Gd)
    ops.join_side_streams()
    assert y.shape == Gd.shape and xg.grad.shape == xg.shape and wg.grad.shape == wg.shape
    assert y.dtype == xg.grad.dtype == wg.grad.dtype == torch.float32
    assert y.is_contiguous() and xg.grad.is_contiguous() and wg.grad.is_contiguous()
    return {"y": y.detach(), "gx": xg.grad, "gw": wg.grad}


def _compare(label, paths, hip, q64, e32, fails, parts):
    """Module-docstring rule for every quantity; prints the ratios, collects the failures (asserted after all prints)."""
    for k, got in hip.items():
        ref = q64[k]
        err = float((got.cpu().double() - ref).abs().max())
        scale = float(ref.abs().max())
        bound = K * e32[k] + FLOOR * scale
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"C3RATIO {paths[k]} {k} {ratio:.3f}   # {label}: err {err:.3e}, e32 {e32[k]:.3e} [{parts[k]}], max|ref| {scale:.3e}")
        if not err <= bound:                                     # (a NaN fails)
            fails.append(f"{label}: {k} on {paths[k]}: |hip - fp64| = {err:.3e} > {K} * {e32[k]:.3e} + {FLOOR} * {scale:.3e}"
                         f" (ratio {ratio:.2f})")


def _run_case(ecm, name):
    c = CASES[name]
    x, w, G, Gs = _operands(name, c)
    L = launches(c)
    on_wino = c.op == "conv" and c.stride == 1 and wino_ok(c.dims, c.wino) and not is_c1(c.Co, c.Ci, c.stride)
    # one pass per weight-gradient form the case can take (the forward and the data gradient run again and must not move)
    passes = [True, False] if on_wino or (c.op == "wgrad" and c.stride == 1 and wino_ok(c.dims, c.wino)) else [False]
    fails, runs = [], {}
    try:
        for ww in passes:
            with switches(ecm, c.wino, ww):
                runs[ww] = [_hip(ecm, c, x, w, G, Gs) for _ in range(2)]
        q64 = _torch(c, x, w, G, Gs, torch.float64, "cpu")
        draws = [_torch(c, x, w, G, Gs, torch.float32, "cpu"), _torch(c, x, w, G, Gs, torch.float32, DEV)]
        wdraw = _wino32(c, x, w, G, Gs) if passes[0] else None
        cdraw = _chain32(c, L, x, w, G, Gs)
        for ww in passes:
            a, b = runs[ww]
            paths = {}
            for q, fam, g in L:
                if fam != "wgrad" or (g["kind"] == "wino") == ww:
                    paths[q] = path_name(q, fam, g)
            e32, parts = {}, {}
            for k in a:
                cand = list(draws)
                if wdraw is not None and (k != "gw" or ww) and (k == "gw" or on_wino):
                    cand.append(wdraw)
                if k in cdraw:
                    cand.append(cdraw)
                each = [float((d[k].cpu().double() - q64[k]).abs().max()) for d in cand]
                e32[k], parts[k] = max(each), " ".join("%.2e" % e for e in each)
            label = f"{name} wino_wgrad={int(ww)}"
            _compare(label, paths, a, q64, e32, fails, parts)
            for k in a:
                if not torch.equal(a[k], b[k]):
                    fails.append(f"{label}: {k} differs between two runs in {int((a[k] != b[k]).sum())} elements")
        if len(passes) == 2:                                     # the weight-gradient switch moves nothing else
            for k in ("y", "gx"):
                if k in runs[True][0] and not torch.equal(runs[True][0][k], runs[False][0][k]):
                    fails.append(f"{name}: {k} depends on ops.WINOGRAD_WGRAD")
        ecm.ops.check_async_errors()
        assert not fails, "\n".join(fails)
    finally:
        del runs


# ---- the tests -------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_class():
    assert missing_classes() == []


RESTATEMENT_SHAPES = [(1, 3, 5, (3, 5, 7)), (2, 4, 3, (2, 4, 2)), (1, 2, 2, (1, 3, 6))]     # odd / even H and W, W = 2, odd Ci


@pytest.mark.parametrize("shape", RESTATEMENT_SHAPES, ids=str)
def test_winograd_restatement_is_the_convolution(shape):
    """wino_fwd / wino_dgrad / wino_wgrad in fp64 equal F.conv3d and its autograd in fp64 to 1e-12 of scale: the third candidate of
    the unit evaluates the same operation.  (On the CPU; tests/test_conv3d_geometry.py runs it without a GPU as well.)"""
    B, Ci, Co, dims = shape
    x, w = seeded("c3.rs.x", B, Ci, *dims).double(), seeded("c3.rs.w", Co, Ci, 3, 3, 3).double()
    G = seeded("c3.rs.G", B, Co, *dims).double()
    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv3d(xs, ws, None, 1, 1)
    y.backward(G)
    for got, ref in ((wino_fwd(x, w), y.detach()), (wino_dgrad(G, w), xs.grad), (wino_wgrad(x, G), ws.grad)):
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("stride", [1, 2])
def test_chain_restatement_is_the_convolution(stride):
    """chain_conv / chain_dgrad in fp64 equal F.conv3d and its data gradient in fp64 to 1e-12 of scale (on the CPU)."""
    x, w = seeded("c3.ch.x", 2, 6, 4, 5, 7).double(), seeded("c3.ch.w", 5, 6, 3, 3, 3).double()
    xs = x.clone().requires_grad_()
    y = F.conv3d(xs, w, None, stride, 1)
    G = seeded("c3.ch.G", *y.shape).double()
    y.backward(G)
    pairs = [(chain_conv(x, w, stride, 4), y.detach())] + ([(chain_dgrad(G, w, 4), xs.grad)] if stride == 1 else [])
    for got, ref in pairs:
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv3d_fp64(ecm, name):
    """y, gx and gw of one case of the table on every kernel it dispatches to: the fp64 bound, bit-identical repeats."""
    _run_case(ecm, name)
