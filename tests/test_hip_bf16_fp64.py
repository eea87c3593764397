"""The opt-in bf16 inference convolutions against fp64, on every instantiation of csrc/bf16_encoder.hip (conv2d_bf16),
csrc/bf16_decoder.hip (deconv2d_bf16, conv2d_c1_bf16), csrc/bf16_infer.hip on csrc/bf16_conv3d.h (conv3d_taps<Bf16Op, ..>) and the
bf16 instantiation of the classifier tail in csrc/conv3d_c1.hip (conv3d_c1_fwd_v<true, unsigned short>).

Which instantiation runs is decided silently by the shape (the kind's NT, COT from Co, VEC from W % 8, the output type), and so is
how many chunks the double-buffered loop of bf16_conv2d.h walks and whether a tile is ragged.  The case table below names, for every
instantiation, every phase of the chunk loops and every tile edge, the smallest shape that reaches it; the host-side dispatch is
restated here in Python so that the mapping is asserted (tests/test_bf16_geometry.py pins every constant and dispatch line to its
source and asserts `missing_classes() == []` on the CPU) instead of assumed.  The operations are reached through ecm_amd.ops as the
models reach them: ops.conv2d_bf16 (both output types), ops.deconv2d_k3s2_bias_bf16, ops.conv2d_c1_relu_bf16, ops.conv3d_k3 and
ops.deconv3d_k3s2 on bf16 volumes, ops.classifier_tail on a bf16 volume -- under torch.no_grad(), inside the bf16 block of their
region, with the weight images packed per call (the frozen_weights() cache is out of scope here).

Operands: oracle.weights.seeded under a name per case, weights He-scaled; activations and weights are rounded to bf16 first, so
every product is exact in fp32 and the fp64 reference computes the very expression the kernel does.  Bias, gamma and beta stay
fp32.  Reference: F.conv2d / F.conv_transpose2d / F.conv3d / F.conv_transpose3d (the tail: F.group_norm, ReLU, F.conv3d) in fp64 on
the CPU.  Unit: the reference's OWN fp32 error, e32 = max |y32 - y64| over two independent fp32 evaluations of the same expression,
torch's on the CPU and torch's on the device (TF32 off).  With K = 4 and FLOOR = 2e-7 (those of test_hip_conv3d_fp64.py),
bound = K * e32 + FLOOR * max|y64|, and
  * an fp32 output passes when  max|y - y64| <= bound;
  * a bf16 output is an fp32 accumulator rounded once, to nearest even; rounding is monotone, so a correct kernel satisfies,
    elementwise,  rne_bf16(y64 - bound) <= y <= rne_bf16(y64 + bound).  That is asserted as it stands: no ulp allowance, no
    relative floor.  `rne_bf16` rounds the fp64 bits directly (no detour through fp32, which could move a value onto a tie).
    The share of outputs whose two ends differ ("undecided": the reference alone does not decide the bf16 value) is printed
    and capped at UNDECIDED_CAP = 2 %, so the check cannot degenerate into a 1-ulp test.
The forward of the ReLU (conv2d_c1_relu_bf16 after the sum, the tail's before it) is continuous, so the bound holds through the kink
and nothing is excluded.

Every case runs twice on fresh device copies of its operands, each run after `poison()` (tests/test_hip_costvol_fp64.py: the blocks
the allocator hands out next hold NaN), the two results must be bit-identical and finite, and a case's outputs stay alive until it
ends: an element a ragged tile forgets to write cannot inherit the right value from recycled memory.

Each check prints `BFRATIO <path> <quantity> <ratio>`; for a bf16 output the ratio is the distance by which y lies outside the
interval in units of `bound` (0 inside).  DESIGN.md section 4 holds the worst ratio per family as measured on the MI355X."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle.weights import seeded
from test_hip_conv3d_fp64 import DEV, FLOOR, K, cdiv
from test_hip_costvol_fp64 import poison

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
UNDECIDED_CAP = 0.02
GN_EPS = 1e-5


# ---- the host-side dispatch, restated (tests/test_bf16_geometry.py pins every constant to its source) ---------------------------
KC = 16                                 # bf16_conv2d.h: input channels per chunk of stage2d_run
TW = 32                                 # bf16_encoder.hip, bf16_conv3d.h: output columns per tile
# bf16_encoder.hip dispatch: (k, stride, dil) -> launch_co<k, stride, dil, NT>
ENC_NT = {(3, 1, 1): 2, (3, 1, 2): 2, (3, 1, 4): 1, (3, 2, 1): 1, (1, 1, 1): 2, (1, 2, 1): 2}
DTW, DTH, DIWP = 32, 4, 40              # bf16_decoder.hip: input columns / rows per workgroup of deconv2d_bf16, window columns
C1R, C1W, C1_WAVES, C1MAXW = 4, 512, 4, 9 * 1024      # conv2d_c1_bf16: rows per lane, columns per wave, waves, weights in LDS
# bf16_infer.hip: (TD, TH) of MODE 0 (stride 1), 1 (stride 2), 2 (transposed); bf16_conv3d.h: chunks of 8 channels
TAPS_TILE = {0: (4, 4), 1: (2, 4), 2: (4, 4)}
TAPS_KC = 8
VT_D, VT_H, VT_W = 8, 16, 32            # conv3d_c1.hip: the tail's tile


def geo2(k, stride, dil, nt):
    """Geo2<KS, S, DL, NT> of bf16_encoder.hip"""
    pad = dil * (k - 1) // 2
    th = 4 * nt
    xoff = 8 - pad if pad else 0
    return dict(PAD=pad, TH=th, HR=stride * (th - 1) + dil * (k - 1) + 1, XOFF=xoff,
                IWP=(xoff + stride * (TW - 1) + dil * (k - 1) + 1 + 7) // 8 * 8)


def enc_cot(k, stride, Co):
    """launch_co"""
    if k == 1 and stride == 1 and Co % 128 == 0:
        return 4
    return 2 if Co % 64 == 0 else 1


def conv2d_bf16_supported(Ci, Co, k, stride, dil):
    """ops.conv2d_bf16_supported"""
    if Ci % 16 or Co % 32 or Ci <= 0 or Co <= 0:
        return False
    if k == 3:
        return (stride == 1 and dil in (1, 2, 4)) or (stride == 2 and dil == 1)
    return k == 1 and stride in (1, 2) and dil == 1


def enc_geom(B, Ci, Co, H, W, k, stride, dil, f32):
    """ecm_conv2d_bf16_fwd -> dispatch<OutT> -> launch_co -> launch_enc: the instantiation, its grid, chunk count, raggedness."""
    assert Ci % KC == 0 and Co % 32 == 0 and (k, stride, dil) in ENC_NT, "ECM_EUNSUP"
    nt = ENC_NT[(k, stride, dil)]
    cot = enc_cot(k, stride, Co)
    TH = 4 * nt
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    th, tw = cdiv(Ho, TH), cdiv(Wo, TW)
    return dict(fam="enc", inst=(k, stride, dil, nt, cot, W % 8 == 0, "f32" if f32 else "bf16"), kind=(k, stride, dil), vec=W % 8 == 0,
                grid=(B * th * tw, Co // (32 * cot)), tiles=(th, tw), tile=(TH, TW), out=(Ho, Wo), inp=(H, W), B=B, chunks=Ci // KC)


def dec_geom(B, Ci, Co, H, W):
    """ecm_deconv2d_k3s2_bias_bf16_fwd -> launch_dec<Co / 32>: tiles of DTH x DTW INPUT positions"""
    assert Ci % KC == 0 and Co in (32, 64), "ECM_EUNSUP"
    th, tw = cdiv(H, DTH), cdiv(W, DTW)
    return dict(fam="dec", inst=(Co // 32, W % 8 == 0), vec=W % 8 == 0, grid=(B * th * tw, 1), tiles=(th, tw), tile=(DTH, DTW), out=(H, W),
                inp=(H, W), B=B, chunks=Ci // KC)


def c1_geom(B, Ci, H, W):
    """ecm_conv2d_c1_bf16_fwd: a workgroup is C1_WAVES waves of C1R rows each by C1W columns"""
    assert Ci % KC == 0 and 9 * Ci <= C1MAXW, "ECM_EUNSUP"
    rows = C1_WAVES * C1R
    th, tw = cdiv(H, rows), cdiv(W, C1W)
    return dict(fam="c1", inst=(W % 8 == 0,), vec=W % 8 == 0, grid=(B * th * tw, 1), tiles=(th, tw), tile=(rows, C1W), out=(H, W), inp=(H, W),
                B=B, idle_wave=cdiv(H, C1R) % C1_WAVES != 0, chunks=None)


def taps_geom(B, Ci, Co, D, H, W, mode):
    """ecm_conv3d_k3_bf16_fwd (MODE 0: stride 1, MODE 1: stride 2) and ecm_deconv3d_k3s2_bf16_fwd (MODE 2, which tiles the INPUT
    grid and runs its 8 output phases on blockIdx.y) -> launch_conv3d_taps<Bf16Op, Co / 32, MODE, TD, TH>"""
    assert Ci in (32, 64) and Co in (32, 64), "ECM_EUNSUP"          # taps_channels_ok
    TD, TH = TAPS_TILE[mode]
    s = 2 if mode == 1 else 1
    out = tuple((n - 1) // s + 1 for n in (D, H, W))
    tiles = (cdiv(out[0], TD), cdiv(out[1], TH), cdiv(out[2], TW))
    return dict(fam="taps", inst=(Co // 32, mode, TD, TH), mode=mode, grid=(B * tiles[0] * tiles[1] * tiles[2], 8 if mode == 2 else 1),
                tiles=tiles, tile=(TD, TH, TW), out=out, inp=(D, H, W), B=B, chunks=Ci // TAPS_KC)


def tail_geom(B, D, H, W):
    """ecm_conv3d_c1_gn_fwd_bf16 -> launch_c1_fwd_v<true, unsigned short>"""
    tiles = (cdiv(D, VT_D), cdiv(H, VT_H), cdiv(W, VT_W))
    return dict(fam="tail", inst=("bf16",), grid=(B * tiles[0] * tiles[1] * tiles[2], 1), tiles=tiles, tile=(VT_D, VT_H, VT_W),
                out=(D, H, W), inp=(D, H, W), B=B, chunks=None)


# ---- the case table ------------------------------------------------------------------------------------------------------------
# op: "enc" = ops.conv2d_bf16 (f32: out_dtype fp32), "dec" = ops.deconv2d_k3s2_bias_bf16 (bias: "big" = +-50), "c1" =
# ops.conv2d_c1_relu_bf16, "c3" = ops.conv3d_k3 on a bf16 volume, "dc3" = ops.deconv3d_k3s2 on one, "tail" = ops.classifier_tail.
# dims: the INPUT extents (H, W) or (D, H, W).
Case = collections.namedtuple("Case", "op B Ci Co dims k stride dil f32 bias", defaults=(3, 1, 1, False, None))

ENC_KINDS = tuple(ENC_NT)


def _enc_table():
    """One case per instantiation of conv2d_bf16: kind x COT x VEC x OutT.  The output extents walk four tile archetypes per VEC
    value (in units of the kind's TH x 32 tile; at stride 2 the input extent is 2n or 2n - 1, odd for every 2-byte-load case) and
    the chunk count walks 1, 2, 3, 4, both in the order of the table, so that every archetype and every chunk count meets both
    values of VEC.  B = 2 wherever the archetype says so."""
    vec = (("exact", lambda TH: (1, TH, 32)), ("two_ragged", lambda TH: (1, 2 * TH + 1, 40)), ("ragged", lambda TH: (1, max(TH - 3, 1), 8)),
           ("b2_wide", lambda TH: (2, TH + 1, 64)))
    any_ = (("two_ragged", lambda TH: (1, 2 * TH + 1, 41)), ("b2_one_past", lambda TH: (2, TH + 1, 33)), ("ragged", lambda TH: (1, 3, 5)),
            ("wide", lambda TH: (1, TH, 35)))
    out, n = {}, {True: 0, False: 0}
    for k, stride, dil in ENC_KINDS:
        TH = 4 * ENC_NT[(k, stride, dil)]
        for Co in (32, 64) + ((128,) if (k, stride) == (1, 1) else ()):
            for v in (True, False):
                for f32 in (False, True):
                    j = n[v]
                    n[v] += 1
                    label, fn = (vec if v else any_)[j % 4]
                    B, Ho, Wo = fn(TH)
                    H = Ho if stride == 1 else (2 * Ho - 1 if (j // 4) % 2 == 0 or not v else 2 * Ho)
                    W = Wo if stride == 1 else (2 * Wo if v else 2 * Wo - 1)
                    Ci = KC * (1 + (j + j // 4) % 4)
                    name = "e_k%ds%dd%d_co%d_%s_%s_%s" % (k, stride, dil, Co, "vec" if v else "any", "f32" if f32 else "bf16", label)
                    out[name] = Case("enc", B, Ci, Co, (H, W), k, stride, dil, f32)
    return out


ENC = _enc_table()
ENC_EDGES = {
    # extent 1; dilation 2 and 4 on a map narrower and lower than the dilation: every tap but the centre one reads padding
    "e_one": Case("enc", 1, 16, 32, (1, 1)),
    "e_one_1x1s2": Case("enc", 2, 32, 64, (1, 1), 1, 2, 1, True),
    "e_d2_all_halo": Case("enc", 1, 32, 32, (1, 1), 3, 1, 2),
    "e_d4_all_halo": Case("enc", 1, 48, 64, (3, 3), 3, 1, 4, True),
    # cb > 0: the grid's y extent Co / (32 * COT) is 3, 2, 2
    "e_cb_co96": Case("enc", 1, 16, 96, (5, 9)),                                    # COT 1, three channel blocks
    "e_cb_co128_s2": Case("enc", 1, 32, 128, (9, 17), 3, 2, 1, True),               # COT 2, two channel blocks; odd extents at stride 2
    "e_cb_co256_1x1": Case("enc", 2, 16, 256, (3, 8), 1, 1, 1),                     # COT 4, two channel blocks
}
DEC = {
    # deconv2d_bf16<Co / 32, VEC>: tiles of 4 x 32 input positions; 1 .. 4 chunks for each VEC
    "d_exact": Case("dec", 1, 16, 32, (4, 32)),
    "d_two_ragged_vec": Case("dec", 1, 32, 64, (9, 40)),
    "d_ragged_vec": Case("dec", 1, 48, 64, (3, 8)),
    "d_four_chunks_vec": Case("dec", 2, 64, 32, (4, 40)),
    "d_two_ragged": Case("dec", 1, 48, 32, (9, 41)),
    "d_b2_one_past": Case("dec", 2, 64, 64, (5, 33)),
    "d_ragged": Case("dec", 1, 16, 64, (3, 5)),
    "d_two_chunks": Case("dec", 1, 32, 32, (5, 35)),
    "d_one": Case("dec", 1, 16, 32, (1, 1)),
    "d_bias50": Case("dec", 1, 32, 64, (5, 33), bias="big"),                        # a bias added after the rounding fails the interval
}
C1 = {
    # conv2d_c1_bf16<VEC>: 4 waves x 4 rows by 512 columns
    "c1_one": Case("c1", 4, 16, 1, (1, 1)),                                         # extent 1 (B = 4: the ReLU sees both sides)
    "c1_w520": Case("c1", 1, 16, 1, (5, 520)),                                      # W crosses 512; H % 4 != 0; waves 2, 3: r0 >= H
    "c1_w517": Case("c1", 1, 32, 1, (6, 517)),                                      # the same crossing with 2-byte loads
    "c1_exact": Case("c1", 1, 16, 1, (16, 512)),
    "c1_h17": Case("c1", 2, 16, 1, (17, 9)),                                        # H > 16: a second tile row of one row
    "c1_h19_vec": Case("c1", 1, 16, 1, (19, 8)),
}
TAPS = {
    # conv3d_taps<Bf16Op, Co / 32, MODE 0, 4, 4>
    "t_s1_ragged": Case("c3", 1, 32, 32, (3, 3, 5)),
    "t_s1_exact": Case("c3", 1, 64, 32, (4, 4, 32)),
    "t_s1_two_ragged": Case("c3", 1, 64, 64, (5, 5, 33)),
    "t_s1_one": Case("c3", 2, 32, 64, (1, 1, 1)),
    # MODE 1, tiles of 2 x 4 x 32 outputs
    "t_s2_odd": Case("c3", 1, 32, 32, (5, 7, 65), stride=2),                        # -> 3 x 4 x 33
    "t_s2_exact": Case("c3", 2, 64, 32, (4, 8, 64), stride=2),                      # -> 2 x 4 x 32
    "t_s2_two_ragged": Case("c3", 1, 64, 64, (9, 9, 40), stride=2),                 # -> 5 x 5 x 20
    "t_s2_ragged": Case("c3", 1, 32, 64, (1, 5, 9), stride=2),                      # -> 1 x 3 x 5
    "t_s2_one": Case("c3", 1, 64, 64, (1, 1, 1), stride=2),
    # MODE 2, tiles of 4 x 4 x 32 INPUT voxels, 8 phases each
    "t_dc_ragged": Case("dc3", 1, 32, 32, (3, 3, 5)),
    "t_dc_exact": Case("dc3", 1, 64, 32, (4, 4, 32)),
    "t_dc_two_ragged": Case("dc3", 1, 64, 64, (5, 5, 33)),
    "t_dc_one": Case("dc3", 2, 32, 64, (1, 1, 1)),
}
TAIL = {
    # conv3d_c1_fwd_v<true, unsigned short>: tiles of 8 x 16 x 32
    "tail_one": Case("tail", 2, 32, 1, (1, 1, 1)),                                  # (F.group_norm refuses ONE value per channel in all)
    "tail_ragged": Case("tail", 1, 32, 1, (3, 5, 7)),
    "tail_exact": Case("tail", 1, 32, 1, (8, 16, 32)),
    "tail_two_ragged": Case("tail", 1, 32, 1, (9, 17, 33)),
}
CASES = {**ENC, **ENC_EDGES, **DEC, **C1, **TAPS, **TAIL}
# per-case salt of the operand names, where the plain name misses a condition on the operands (tests/test_bf16_geometry.py)
SALT = {"t_s2_one": "#1", "t_s1_ragged": "#1"}


def geom(c):
    if c.op == "enc":
        return enc_geom(c.B, c.Ci, c.Co, *c.dims, c.k, c.stride, c.dil, c.f32)
    if c.op == "dec":
        return dec_geom(c.B, c.Ci, c.Co, *c.dims)
    if c.op == "c1":
        return c1_geom(c.B, c.Ci, *c.dims)
    if c.op in ("c3", "dc3"):
        return taps_geom(c.B, c.Ci, c.Co, *c.dims, 2 if c.op == "dc3" else c.stride - 1)
    return tail_geom(c.B, *c.dims)


def bf16_out(c):
    return not (c.op in ("c1", "tail") or (c.op == "enc" and c.f32))


def path_name(g):
    if g["fam"] == "enc":
        return "conv2d_bf16<%d,%d,%d,%d,%d,%s,%s>" % tuple(str(v).lower() if isinstance(v, bool) else v for v in g["inst"])
    if g["fam"] == "dec":
        return "deconv2d_bf16<%d,%s>" % (g["inst"][0], str(g["inst"][1]).lower())
    if g["fam"] == "c1":
        return "conv2d_c1_bf16<%s>" % str(g["inst"][0]).lower()
    if g["fam"] == "taps":
        return "conv3d_taps<Bf16Op,%d,%d,%d,%d>" % g["inst"]
    return "conv3d_c1_fwd_v<true,bf16>"


def all_instantiations():
    out = []
    for k, stride, dil in ENC_KINDS:
        nt = ENC_NT[(k, stride, dil)]
        for cot in (1, 2) + ((4,) if (k, stride) == (1, 1) else ()):
            out += [("enc", (k, stride, dil, nt, cot, v, o)) for v in (True, False) for o in ("bf16", "f32")]
    out += [("dec", (cot, v)) for cot in (1, 2) for v in (True, False)]
    out += [("c1", (v,)) for v in (True, False)]
    out += [("taps", (ct, mode) + TAPS_TILE[mode]) for mode in (0, 1, 2) for ct in (1, 2)]
    return out + [("tail", ("bf16",))]


def missing_classes():
    """The classes of the issue's list that NO case reaches under the restated dispatch."""
    G = {name: geom(c) for name, c in CASES.items()}
    want = {}
    for fam, inst in all_instantiations():
        want["instantiation %s %s" % (fam, inst)] = any(g["fam"] == fam and g["inst"] == inst for g in G.values())
    for fam in ("enc", "dec"):
        for v in (True, False):
            for n in (1, 2, 3, 4):
                want["stage2d_run of %s, VEC %s: %s chunk(s)" % (fam, v, n if n < 4 else ">= 4")] = any(
                    g["fam"] == fam and g["vec"] == v and (g["chunks"] == n if n < 4 else g["chunks"] >= 4) for g in G.values())
    for mode in (0, 1, 2):
        for n in (4, 8):
            want["conv3d_taps_body MODE %d: %d chunks" % (mode, n)] = any(g["fam"] == "taps" and g["mode"] == mode and g["chunks"] == n
                                                                          for g in G.values())
    for fam in ("enc", "dec", "c1", "taps", "tail"):
        k = [g for g in G.values() if g["fam"] == fam]
        axes = range(len(k[0]["tile"]))
        rag = lambda g, a: g["out"][a] % g["tile"][a] != 0                              # noqa: E731
        want[fam + ": a single ragged tile"] = any(all(t == 1 for t in g["tiles"]) and all(rag(g, a) for a in axes) for g in k)
        want[fam + ": an exact tile"] = any(g["out"] == g["tile"] for g in k)
        for a in axes:
            want[fam + ": more than one tile along axis %d" % a] = any(g["tiles"][a] > 1 for g in k)
            want[fam + ": a ragged last tile after a full one along axis %d" % a] = any(g["tiles"][a] > 1 and rag(g, a) for g in k)
        want[fam + ": B > 1"] = any(g["B"] > 1 for g in k)
        want[fam + ": extent 1"] = any(all(n == 1 for n in g["inp"]) for g in k)
    enc = [g for g in G.values() if g["fam"] == "enc"]
    for cot in (1, 2, 4):
        want["conv2d_bf16: cb > 0 at COT %d" % cot] = any(g["grid"][1] > 1 and g["inst"][4] == cot for g in enc)
    for kind in ((3, 2, 1), (1, 2, 1)):
        want["conv2d_bf16 %s: odd input extents" % (kind,)] = any(g["kind"] == kind and g["inp"][0] % 2 and g["inp"][1] % 2 and g["inp"][0] > 1
                                                                 for g in enc)
        want["conv2d_bf16 %s: even input extents" % (kind,)] = any(g["kind"] == kind and not g["inp"][0] % 2 and not g["inp"][1] % 2 for g in enc)
    for dil in (2, 4):
        want["conv2d_bf16 dilation %d: the map is narrower and lower than the dilation" % dil] = any(
            g["kind"] == (3, 1, dil) and max(g["inp"]) < dil for g in enc)
    want["conv3d_taps stride 2: odd input extents"] = any(g["fam"] == "taps" and g["mode"] == 1 and all(n % 2 and n > 1 for n in g["inp"])
                                                          for g in G.values())
    want["conv3d_taps stride 2: even input extents"] = any(g["fam"] == "taps" and g["mode"] == 1 and not any(n % 2 for n in g["inp"])
                                                           for g in G.values())
    c1 = [g for g in G.values() if g["fam"] == "c1"]
    for v in (True, False):
        want["conv2d_c1_bf16<%s>: W crosses 512" % v] = any(g["vec"] == v and g["inp"][1] > C1W for g in c1)
    want["conv2d_c1_bf16: H % 4 != 0"] = any(g["inp"][0] % C1R for g in c1)
    want["conv2d_c1_bf16: H > 16"] = any(g["inp"][0] > C1_WAVES * C1R for g in c1)
    want["conv2d_c1_bf16: a wave whose r0 >= H"] = any(g["idle_wave"] for g in c1)
    want["deconv2d_bf16: a bias of magnitude 50"] = any(c.op == "dec" and c.bias == "big" for c in CASES.values())
    return sorted(k for k, ok in want.items() if not ok)


# ---- operands, references ----------------------------------------------------------------------------------------------------------
def operands(name):
    """dict(x, w[, b][, gamma, beta]) on the CPU: x bf16; w fp32 holding bf16 values; b, gamma, beta fp32."""
    c = CASES[name]
    n = "bf." + name + SALT.get(name, "")
    x = seeded(n + ".x", c.B, c.Ci, *c.dims).to(BF)
    he = lambda *shape, fan: (seeded(n + ".w", *shape) * (2.0 / fan) ** 0.5).to(BF).float()      # noqa: E731
    if c.op == "enc":
        return dict(x=x, w=he(c.Co, c.Ci, c.k, c.k, fan=c.k * c.k * c.Ci))
    if c.op == "dec":
        b = 50.0 * torch.sign(seeded(n + ".b", c.Co)) if c.bias == "big" else seeded(n + ".b", c.Co) * 0.5
        return dict(x=x, w=he(c.Ci, c.Co, 3, 3, fan=9 * c.Ci), b=b)
    if c.op == "c1":
        w = he(1, c.Ci, 3, 3, fan=9 * c.Ci)
        # the bias sits at the median of the sums, so that the ReLU clamps about half of the outputs
        b = -torch.quantile(F.conv2d(x.double(), w.double(), None, 1, 1).flatten(), 0.5).float().reshape(1)
        return dict(x=x, w=w, b=b)
    if c.op == "c3":
        return dict(x=x, w=he(c.Co, c.Ci, 3, 3, 3, fan=27 * c.Ci))
    if c.op == "dc3":
        return dict(x=x, w=he(c.Ci, c.Co, 3, 3, 3, fan=27 * c.Ci))
    return dict(x=x, w=he(1, 32, 3, 3, 3, fan=27 * 32), gamma=1.0 + 0.2 * seeded(n + ".gamma", 32), beta=0.2 * seeded(n + ".beta", 32))


def torch_forward(c, o, dtype, device):
    """The operation in `dtype` on `device` through torch's own kernels."""
    t = {k: v.to(device=device, dtype=dtype) for k, v in o.items()}
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, allow_tf32=False):
        if c.op == "enc":
            return F.conv2d(t["x"], t["w"], None, c.stride, c.dil * (c.k - 1) // 2, c.dil)
        if c.op == "dec":
            return F.conv_transpose2d(t["x"], t["w"], t["b"], 2, 1, 1)
        if c.op == "c1":
            return F.relu(F.conv2d(t["x"], t["w"], t["b"], 1, 1))
        if c.op == "c3":
            return F.conv3d(t["x"], t["w"], None, c.stride, 1)
        if c.op == "dc3":
            return F.conv_transpose3d(t["x"], t["w"], None, 2, 1, 1)
        return F.conv3d(F.relu(F.group_norm(t["x"], 32, t["gamma"], t["beta"], GN_EPS)), t["w"], None, 1, 1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(operands, y64, y32 on the CPU) of a case: computed once, shared by the tests, never written to."""
    o = operands(name)
    return o, torch_forward(CASES[name], o, torch.float64, "cpu"), torch_forward(CASES[name], o, torch.float32, "cpu")


def rne_bf16(v):
    """The bf16 value nearest to each fp64 v (ties to even), as fp64, from the fp64 bits themselves: a bf16 has 8 significant
    bits, so the low 45 bits of the fp64 significand are rounded away in integer arithmetic (a carry runs into the exponent
    field, which is the next binade's first value).  Going through fp32 instead would round twice: a value just above a bf16
    tie can land ON the tie in fp32 and then go to even, the wrong way.  Below 2^-126 a bf16 is denormal with a fixed spacing of
    2^-133; the result is exactly representable in bf16, so later casts to fp32 or bf16 do not change it."""
    bits = v.contiguous().view(torch.int64)
    r = ((bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) >> 45) << 45
    sub = torch.round(v * 2.0 ** 133) * 2.0 ** -133                 # torch.round: half to even
    return torch.where(v.abs() < 2.0 ** -126, sub, r.view(torch.float64))


def interval(y64, bound):
    return rne_bf16(y64 - bound), rne_bf16(y64 + bound)


def cpu_conditions(name):
    """The operand conditions that need no GPU: dict(undecided share with b0 = K * e32(CPU) + FLOOR * max|y64| for a bf16-output
    case, share of positive outputs for a conv2d_c1_relu_bf16 case)."""
    c = CASES[name]
    _, y64, y32 = reference(name)
    out = {}
    if bf16_out(c):
        b0 = K * float((y32.double() - y64).abs().max()) + FLOOR * float(y64.abs().max())
        lo, hi = interval(y64, b0)
        out["undecided"] = float((lo != hi).double().mean())
    if c.op == "c1":
        out["positive"] = float((y64 > 0).double().mean())
    return out


# ---- the device side --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def _hip(ecm, c, o):
    """The operation through ecm_amd.ops on fresh device copies of the operands, after poisoning what the allocator hands out."""
    ops = ecm.ops
    poison()
    t = {k: v.to(DEV, copy=True) for k, v in o.items()}
    region = {"enc": ops.encoder_dtype, "dec": ops.decoder_dtype, "c1": ops.decoder_dtype}.get(c.op, ops.aggregation_dtype)
    with torch.no_grad(), region(BF):
        if c.op == "enc":
            y = ops.conv2d_bf16(t["x"], t["w"], c.stride, c.dil, out_dtype=torch.float32 if c.f32 else BF)
        elif c.op == "dec":
            y = ops.deconv2d_k3s2_bias_bf16(t["x"], t["w"], t["b"])
        elif c.op == "c1":
            y = ops.conv2d_c1_relu_bf16(t["x"], t["w"], t["b"])
        elif c.op == "c3":
            y = ops.conv3d_k3(t["x"], t["w"], c.stride)
        elif c.op == "dc3":
            y = ops.deconv3d_k3s2(t["x"], t["w"])
        else:
            y = ops.classifier_tail(t["x"], t["gamma"], t["beta"], t["w"])
    torch.cuda.synchronize()
    return y


def _run_case(ecm, name):
    c = CASES[name]
    g = geom(c)
    path = path_name(g)
    o, y64, y32 = reference(name)
    runs = None
    try:
        runs = [_hip(ecm, c, o) for _ in range(2)]
        a, b = runs
        ecm.ops.check_async_errors()
        assert a.shape == y64.shape and a.is_contiguous() and a.dtype == (BF if bf16_out(c) else torch.float32), (a.shape, a.dtype)
        y = a.cpu().double()
        fails = []
        if not bool(torch.isfinite(y).all()):
            fails.append(f"{name}: {int((~torch.isfinite(y)).sum())} outputs are not finite")
        if not torch.equal(a, b):
            fails.append(f"{name}: the output differs between two runs in {int((a != b).sum())} elements")
        each = [float((y32.double() - y64).abs().max()), float((torch_forward(c, o, torch.float32, DEV).cpu().double() - y64).abs().max())]
        e32, scale = max(each), float(y64.abs().max())
        bound = K * e32 + FLOOR * scale
        parts = " ".join("%.2e" % e for e in each)
        if bf16_out(c):
            lo, hi = interval(y64, bound)
            out = torch.clamp(torch.maximum(lo - y, y - hi), min=0.0)
            err, undecided = float(out.max()), float((lo != hi).double().mean())
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            print(f"BFRATIO {path} y_bf16 {ratio:.3f}   # {name}: outside by {err:.3e}, undecided {undecided:.3%}, e32 {e32:.3e} [{parts}], "
                  f"max|ref| {scale:.3e}")
            if not err == 0:                                             # (a NaN fails)
                bad = int((out > 0).sum())
                fails.append(f"{name}: {path}: {bad} outputs lie outside [rne_bf16(y64 - b), rne_bf16(y64 + b)], b = {K} * {e32:.3e} + "
                             f"{FLOOR} * {scale:.3e}, by up to {err:.3e} (ratio {ratio:.2f})")
            if not undecided <= UNDECIDED_CAP:
                fails.append(f"{name}: {undecided:.2%} of the outputs are not decided by the reference (cap {UNDECIDED_CAP:.0%})")
        else:
            err = float((y - y64).abs().max())
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            print(f"BFRATIO {path} y_f32 {ratio:.3f}   # {name}: err {err:.3e}, e32 {e32:.3e} [{parts}], max|ref| {scale:.3e}")
            if not err <= bound:
                fails.append(f"{name}: {path}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")
        assert not fails, "\n".join(fails)
    finally:
        del runs


# ---- the tests -------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_class():
    assert missing_classes() == []


@pytest.mark.parametrize("name", sorted(CASES))
def test_bf16_fp64(ecm, name):
    """One case of the table on the kernel it dispatches to: the fp64 bound or interval, finite outputs, bit-identical repeats."""
    _run_case(ecm, name)
