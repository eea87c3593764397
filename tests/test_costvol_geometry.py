"""The path tables of tests/test_hip_costvol_fp64.py and tests/test_hip_metrics_fp64.py, checked without a GPU.

This module holds what the two GPU suites share and what can be shown on the CPU:

  * the constants of csrc/costvol.hip, costvol_conv.hip, loss.hip and eval.hip that the restated host dispatch uses, pinned to the
    sources as they stand (a retune must not silently move the cases off the paths they were chosen for);
  * `classP` / `classQ` of csrc/costvol_conv.hip restated, and vectorised closed forms in plain torch that follow the dtype and
    device of their input: `class_weights_t` (the 0/1 tap-mask einsum), `assemble_t` (a gather), `collapsed_t` (both composed with
    two 2-D convolutions written as sums over taps) and `cost_volume_t`;  `collapsed_t` equals
    F.conv3d(O.cost_volume(L, R, D), W) in fp64 to 1e-12 of scale on a grid of small shapes, and the classes that can occur are
    exactly 13 of the 15 reference-half ones (9 and 12 -- d - x of 1 or 2 at the first plane, i.e. x < 0 -- never do) and all 6
    target-half ones;
  * the case tables with `classes_of` / `missing_classes` (which must be empty) and the smallest case per class;
  * the threshold tables of the loss and of the EPE (`loss_table`, `epe_table`): operands on a dyadic grid such that every fp32
    difference the kernels take (p - gt, pred - d, x - d) is exact, so a decision boundary is met exactly and not merely approached.
"""
import collections
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import oracle.ecm_oracle as O
from conftest import ROOT
from oracle.weights import seeded

CSRC = os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc")

# ---- constants of the sources (pinned below) ----------------------------------------------------------------------------------------
SEG, THREADS, GRID_Y_MAX = 1024, 256, 65535        # costvol.hip: floats per segment, threads, the largest B*C the v4 grid takes
NCP, NCQ = 15, 6                                   # costvol_conv.hip: classes of the reference / target half
LDS_MAX = 64 * 1024                                # costvol_conv.hip: both row-staged gates
LT = ET = 256                                      # loss.hip / eval.hip: threads of a reduction workgroup
PER_THREAD, MAX_BLOCKS, FINAL_LANES = 8, 1024, 64  # elements per thread below the cap, the cap, lanes of stereo_loss_final
CHUNK = 32                                         # eval.hip U16_MAXB / frame_io.h FP_MAXB: samples per launch
UNREACHABLE_P = (9, 12)
MAXDISP = 192.0


def cdiv(a, b):
    return -(-a // b)


# ---- host-side dispatch, restated ------------------------------------------------------------------------------------------------
def dpad(D):
    return ((D + 3) // 4 + 1) * 4


def concat_path(B, C, w):
    return "v4" if w % 4 == 0 and B * C <= GRID_Y_MAX else "scalar"


def fwd_lds_bytes(w):
    return (NCP * w + NCQ * (w + 2)) * 4          # = (21 w + 12) * 4


def bwd_lds_bytes(D, w):
    return D * w * 4


def assemble_fwd_path(w, aligned):
    if w % 4 == 0 and aligned and fwd_lds_bytes(w) <= LDS_MAX:
        return "rows"
    return "vec4" if w % 4 == 0 else "scalar"


def assemble_bwd_path(D, w, aligned):
    return "rows" if w % 4 == 0 and aligned and bwd_lds_bytes(D, w) <= LDS_MAX else "elementwise"


def reduce_blocks(n):
    """loss_blocks / eval_blocks."""
    return max(1, min(MAX_BLOCKS, cdiv(n, LT * PER_THREAD)))


def edge_of(d, D):
    return 0 if d == 0 else (2 if d == D - 1 else 1)


def classP(d, x, D):
    """Class of the reference half at (d, x); None where d - x >= 3 (no tap passes the wedge: y = 0)."""
    delta = d - x
    if delta >= 3:
        return None
    return (max(delta, -2) + 2) * 3 + edge_of(d, D)


def classQ(d, x, D, w):
    return edge_of(d, D) * 2 + (1 if x == w - 1 else 0)


def classes_touched(w, D):
    P = {classP(d, x, D) for d in range(D) for x in range(w)} - {None}
    Q = {classQ(d, x, D, w) for d in range(D) for x in range(w) if d - x < 3}
    return P, Q


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def tap_masks(dtype=torch.float32, device="cpu"):
    """mP [15,kd,kw], mQ [6,kd,kw,ku]: which taps of the 3x3x3 kernel a class keeps (header of csrc/costvol_conv.hip)."""
    mP, mQ = torch.zeros(NCP, 3, 3, dtype=dtype), torch.zeros(NCQ, 3, 3, 5, dtype=dtype)
    for e in range(3):
        for kd in range(3):
            if (e == 0 and kd == 0) or (e == 2 and kd == 2):
                continue                                     # depth padding at the first / last disparity plane
            for kw in range(3):
                for dc in range(5):
                    if kw - kd >= dc - 2:                    # the wedge `x >= d` at the tap
                        mP[dc * 3 + e, kd, kw] = 1
                mQ[e * 2, kd, kw, kw - kd + 2] = 1
                if kw != 2:
                    mQ[e * 2 + 1, kd, kw, kw - kd + 2] = 1   # right border column: the tap to the right is outside
    return mP.to(device), mQ.to(device)


def class_weights_t(W):
    """[Co,2C,3,3,3] -> (wP [15Co,C,3,3], wQ [6Co,C,3,5])."""
    Co, C = W.shape[0], W.shape[1] // 2
    mP, mQ = tap_masks(W.dtype, W.device)
    wP = torch.einsum("xdk,oidhk->xoihk", mP, W[:, :C]).reshape(NCP * Co, C, 3, 3)
    wQ = torch.einsum("xdkq,oidhk->xoihq", mQ, W[:, C:]).reshape(NCQ * Co, C, 3, 5)
    return wP, wQ


def class_index(D, w, device="cpu"):
    """(cp [D,w], cq [D,w], j [D,w] = x - d + 2 clamped, valid [D,w] = d - x < 3)."""
    d = torch.arange(D, device=device).view(-1, 1)
    x = torch.arange(w, device=device).view(1, -1)
    e = torch.where(d == 0, 0, torch.where(d == D - 1, 2, 1))
    cp = ((d - x).clamp(-2, 2) + 2) * 3 + e
    cq = e * 2 + (x == w - 1).long()
    return cp, cq + 0 * x, (x - d + 2).clamp(min=0), (d - x) < 3


def assemble_t(P, Qp, D):
    """P [B,15Co,h,w], Qp [B,6Co,h,w+2] -> y [B,Co,D,h,w]: one add per element, zero where d - x >= 3."""
    B, c15, h, w = P.shape
    Co = c15 // NCP
    cp, cq, j, valid = class_index(D, w, P.device)
    Pv = P.view(B, NCP, Co, h, w).permute(0, 2, 3, 1, 4)                                     # [B,Co,h,15,w]
    Qv = Qp.view(B, NCQ, Co, h, w + 2).permute(0, 2, 3, 1, 4).reshape(B, Co, h, NCQ * (w + 2))
    p = torch.gather(Pv, 3, cp.expand(B, Co, h, D, w))
    q = torch.gather(Qv, 3, (cq * (w + 2) + j).view(1, 1, 1, D * w).expand(B, Co, h, D * w)).view(B, Co, h, D, w)
    y = torch.where(valid, p + q, torch.zeros((), dtype=P.dtype, device=P.device))
    return y.permute(0, 1, 3, 2, 4).contiguous()


def conv2d_taps(x, wt, pad_left, pad_right):
    """Stride-1 2-D cross-correlation with one row of zero padding above and below, as a sum over taps (no library convolution)."""
    kh, kw = wt.shape[-2:]
    h = x.shape[-2]
    xp = F.pad(x, (pad_left, pad_right, 1, 1))
    wo = xp.shape[-1] - kw + 1
    y = 0
    for a in range(kh):
        for b in range(kw):
            y = y + torch.einsum("oc,bchw->bohw", wt[:, :, a, b], xp[..., a:a + h, b:b + wo])
    return y


def collapsed_t(L, R, W, D):
    """conv3d(cost_volume(L, R, D), W, pad 1) as ops.costvol_conv3d composes it: class weights, a 3x3 convolution of L, the sheared
    3x5 convolution of R with two more zero columns on the left (output width w + 2), the assembly."""
    wP, wQ = class_weights_t(W)
    return assemble_t(conv2d_taps(L, wP, 1, 1), conv2d_taps(R, wQ, 4, 2), D)


def cost_volume_t(L, R, D):
    """O.cost_volume without the loop over d."""
    w = L.shape[-1]
    d = torch.arange(D, device=L.device).view(-1, 1)
    x = torch.arange(w, device=L.device).view(1, -1)
    ok, idx = x >= d, (x - d).clamp(min=0)
    zero = torch.zeros((), dtype=L.dtype, device=L.device)
    Lh = torch.where(ok.view(1, 1, D, 1, w), L.unsqueeze(2), zero)
    Rh = torch.where(ok.view(1, 1, D, 1, w), R[..., idx].permute(0, 1, 3, 2, 4), zero)
    return torch.cat([Lh, Rh], 1).contiguous()


# ---- case tables -------------------------------------------------------------------------------------------------------------------
CCase = collections.namedtuple("CCase", "B C h w D")                  # cost_volume
ACase = collections.namedtuple("ACase", "B Co D h w off")             # assembly; off: operands 4 bytes past a 16-byte boundary
KCase = collections.namedtuple("KCase", "Co C")                       # class weights
XCase = collections.namedtuple("XCase", "B h w D")                    # costvol_conv3d, weight [32,64,3,3,3]
LCase = collections.namedtuple("LCase", "n")                          # stereo_loss3
ECase = collections.namedtuple("ECase", "B Hp Wp Hg Wg ch cw")        # eval_epe

CONCAT = {
    "cv_one_thread": CCase(1, 2, 1, 4, 2),
    "cv_d7": CCase(1, 3, 5, 12, 7),                    # hw = 60: one segment, D % 4 = 3
    "cv_two_segments": CCase(2, 2, 90, 12, 5),         # hw = 1080: a row straddles the cut, the halo reaches into segment 0
    "cv_d_gt_w": CCase(1, 2, 3, 8, 13),
    "cv_long_row": CCase(1, 1, 2, 1028, 6),
    "cv_d8": CCase(2, 3, 4, 16, 8),                    # D % 4 = 0
    "cv_scalar_w13": CCase(1, 3, 7, 13, 5),
    "cv_scalar_w1": CCase(1, 2, 2, 1, 3),
    "cv_grid_limit_scalar": CCase(1, 65536, 1, 4, 2),
    "cv_grid_limit_v4": CCase(1, 65535, 1, 4, 2),
}
_ASM = {
    "w1": (1, 2, 3, 2, 1), "w2": (1, 2, 4, 2, 2), "w3": (1, 1, 2, 1, 3), "w5": (2, 1, 3, 2, 5),
    "w4_d2": (1, 2, 2, 2, 4), "w4_d3": (1, 1, 3, 1, 4), "w4_d4": (2, 1, 4, 1, 4), "w8_d3": (1, 2, 3, 3, 8),
    "w4_d8": (1, 1, 8, 2, 4), "w8_d12": (1, 1, 12, 1, 8), "w12_d8": (1, 2, 8, 1, 12), "w5_d9": (1, 1, 9, 1, 5), "w9_d5": (1, 1, 5, 2, 9),
    "w776": (1, 1, 2, 1, 776), "w780": (1, 1, 2, 1, 780), "d64_w256": (1, 1, 64, 1, 256), "d64_w260": (1, 1, 64, 1, 260),
    "w1028": (2, 2, 3, 2, 1028),
}
ASSEMBLY = {}
for _k, _v in _ASM.items():
    ASSEMBLY["as_" + _k] = ACase(*_v, False)
    if _v[4] % 4 == 0:
        ASSEMBLY["as_" + _k + "_off"] = ACase(*_v, True)
WEIGHTS = {"cw_1x1": KCase(1, 1), "cw_8x12": KCase(8, 12), "cw_3x5": KCase(3, 5), "cw_32x32": KCase(32, 32)}
WHOLE = {"cc_w1": XCase(1, 1, 1, 2), "cc_w2": XCase(1, 2, 2, 3), "cc_w9": XCase(2, 3, 9, 5), "cc_w12_d16": XCase(1, 2, 12, 16),
         "cc_w780": XCase(1, 1, 780, 2)}
LOSS = {"loss_n%d" % n: LCase(n) for n in (1, 63, 255, 2048, 2049, 64 * 2048, 64 * 2048 + 5, 1024 * 2048, 1024 * 2048 + 2049)}
EPE = {
    "epe_tiny": ECase(1, 3, 9, 4, 11, 2, 7),                       # 14 elements; Hp < Hg, Wp < Wg, crop smaller than both
    "epe_one_wg": ECase(1, 9, 260, 8, 300, 8, 256),                # 2048: one full workgroup's share
    "epe_two_wgs": ECase(1, 4, 700, 3, 683, 3, 683),               # 2049
    "epe_many": ECase(3, 70, 330, 75, 320, 64, 300),               # 57600: 29 partials, the last one ragged
    "epe_at_cap": ECase(2, 1024, 1030, 1030, 1024, 1024, 1024),    # 1024 workgroups of 8 elements per thread
    "epe_past_cap": ECase(2, 1030, 1100, 1025, 1040, 1024, 1025),  # 1025 shares on 1024 workgroups: some threads walk 9
}
U16 = dict(B=33, Hp=6, Wp=9)
KITTI_PREP = dict(B=33, H=5, W=7, th=8, tw=12)
CASES = {**CONCAT, **ASSEMBLY, **WEIGHTS, **WHOLE, **LOSS, **EPE}


def _reduce_classes(fam, n, lanes):
    nb = reduce_blocks(n)
    out = {(fam, "fewer-than-one-workgroup") if n < LT else (fam, "at-least-one-workgroup")}
    if n % (LT * PER_THREAD) and nb < MAX_BLOCKS:
        out.add((fam, "ragged-last-workgroup"))
    if lanes:
        out.add((fam, "partials<=%d" % lanes if nb <= lanes else "partials>%d" % lanes))
        if nb == lanes:
            out.add((fam, "partials==%d" % lanes))
    if nb == MAX_BLOCKS:
        out.add((fam, "cap-exact" if n == MAX_BLOCKS * LT * PER_THREAD else "cap-threads-walk-more-than-8"))
        assert n <= MAX_BLOCKS * LT * PER_THREAD or cdiv(n, MAX_BLOCKS * LT) > PER_THREAD
    return out


def classes_of(c):
    """The path classes one case reaches."""
    out = set()
    if isinstance(c, CCase):
        B, C, h, w, D = c
        hw, path = h * w, concat_path(c.B, c.C, c.w)
        if path == "scalar":
            out.add(("concat", "scalar", "w%4" if w % 4 else "grid-limit"))
            if B * C * hw > 256:
                out.add(("concat", "scalar", "more-than-one-workgroup"))
            return out
        out |= {("concat", "v4"), ("concat", "v4", "D%%4=%d" % (D % 4)), ("concat", "v4", "halo-before-plane-start")}
        assert dpad(D) >= D + 3 and dpad(D) % 4 == 0
        if B * C == GRID_Y_MAX:
            out.add(("concat", "v4", "at-grid-limit"))
        if hw == 4:
            out.add(("concat", "v4", "single-thread"))
        if hw % SEG:
            out.add(("concat", "v4", "early-return-threads"))
        if hw > SEG:
            out.add(("concat", "v4", "two-segments"))
            if SEG % w and w < SEG:
                out.add(("concat", "v4", "row-straddles-segment"))
            # a disparity d >= 1 that the first pixels of segment 1 keep (x >= d) and whose source lies in segment 0
            if any((SEG + k) % w >= d > k for k in range(0, min(w, hw - SEG), 4) for d in range(1, D)):
                out.add(("concat", "v4", "halo-into-previous-segment"))
        if w > SEG:
            out.add(("concat", "v4", "row-longer-than-segment"))
        if D > w:
            out.add(("concat", "v4", "D>w"))
        if B > 1:
            out.add(("concat", "v4", "B>1"))
    elif isinstance(c, (ACase, XCase)):
        if isinstance(c, ACase):
            B, Co, D, h, w, off = c
            fams = ("asm-fwd", "asm-bwd")
            fp, bp = assemble_fwd_path(w, not off), assemble_bwd_path(D, w, not off)
            why_f = "" if fp != "vec4" else ("-misaligned" if off and fwd_lds_bytes(w) <= LDS_MAX else "-lds")
            why_b = "" if bp == "rows" else ("-w%4" if w % 4 else "-misaligned" if off and bwd_lds_bytes(D, w) <= LDS_MAX else "-lds")
            out |= {("asm-fwd", fp + why_f), ("asm-bwd", bp + why_b)}
            if fp == "rows":
                if fwd_lds_bytes(w + 4) > LDS_MAX:
                    out.add(("asm-fwd", "rows", "widest-that-fits-lds"))
                if D * (w // 4) > 256 and NCP * (w // 4) > 256:
                    out.add(("asm-fwd", "rows", "second-trip"))
            elif fp == "vec4" and not off and fwd_lds_bytes(w - 4) <= LDS_MAX:
                out.add(("asm-fwd", "vec4", "narrowest-past-lds"))
            if bp == "rows":
                if bwd_lds_bytes(D, w + 4) > LDS_MAX:
                    out.add(("asm-bwd", "rows", "widest-that-fits-lds"))
                if w > 256:
                    out.add(("asm-bwd", "rows", "second-trip"))
            elif w % 4 == 0 and not off and bwd_lds_bytes(D, w - 4) <= LDS_MAX:
                out.add(("asm-bwd", "elementwise", "narrowest-past-lds"))
            if B > 1 and Co > 1 and h > 1 and w > SEG:
                out.add(("asm", "B,Co,h>1-and-w>1024"))
        else:
            B, h, w, D = c
            fams = ("whole",)
            out.add(("whole", "fwd-" + assemble_fwd_path(w, True)))
        P, Q = classes_touched(w, D)
        for fam in fams:
            out |= {(fam, "P", k) for k in P} | {(fam, "Q", k) for k in Q}
            for flag, nm in ((w == 1, "w1"), (w == 2, "w2"), (D == 2, "D2-no-interior-plane"), (D == 3, "D3-one-interior-plane"),
                             (D > w + 2, "D>w+2-all-zero-planes"), (w - 3 >= D - 1 and D >= 3, "all-depth-edges-in-the-every-tap-region")):
                if flag:
                    out.add((fam, nm))
    elif isinstance(c, KCase):
        nP, n = NCP * c.Co * c.C * 9, c.Co * c.C * (NCP * 9 + NCQ * 15)
        out.add(("class-weights", "one-workgroup" if n <= 256 else "several-workgroups"))
        out.add(("class-weights", "a-workgroup-holds-both-branches" if nP % 256 else "branches-split-at-a-workgroup"))
        if 2 * c.Co * c.C * 27 % 256:
            out.add(("class-weights", "bwd-ragged"))
    elif isinstance(c, LCase):
        out |= _reduce_classes("loss", c.n, FINAL_LANES)
    elif isinstance(c, ECase):
        out |= _reduce_classes("epe", c.B * c.ch * c.cw, 0)
        assert c.ch <= min(c.Hp, c.Hg) and c.cw <= min(c.Wp, c.Wg)
        if c.Hp != c.Hg and c.Wp != c.Wg and c.ch < min(c.Hp, c.Hg) and c.cw < min(c.Wp, c.Wg):
            out.add(("epe", "crop-smaller-than-both"))
        if c.ch >= 7:
            out.add(("epe", "every-table-entry-at-columns-0-and-cw-1"))
    return out


def required_classes():
    req = {("concat", "scalar", x) for x in ("w%4", "grid-limit", "more-than-one-workgroup")}
    req |= {("concat", "v4")} | {("concat", "v4", "D%%4=%d" % r) for r in range(4)}
    req |= {("concat", "v4", x) for x in ("halo-before-plane-start", "at-grid-limit", "single-thread", "early-return-threads", "two-segments",
                                          "row-straddles-segment", "halo-into-previous-segment", "row-longer-than-segment", "D>w", "B>1")}
    req |= {("asm-fwd", x) for x in ("rows", "vec4-lds", "vec4-misaligned", "scalar")}
    req |= {("asm-bwd", x) for x in ("rows", "elementwise-lds", "elementwise-misaligned", "elementwise-w%4")}
    req |= {("asm-fwd", "rows", "widest-that-fits-lds"), ("asm-fwd", "vec4", "narrowest-past-lds"), ("asm-fwd", "rows", "second-trip"),
            ("asm-bwd", "rows", "widest-that-fits-lds"), ("asm-bwd", "elementwise", "narrowest-past-lds"), ("asm-bwd", "rows", "second-trip"),
            ("asm", "B,Co,h>1-and-w>1024")}
    reach_p = [k for k in range(NCP) if k not in UNREACHABLE_P]
    for fam in ("asm-fwd", "asm-bwd", "whole"):
        req |= {(fam, "P", k) for k in reach_p} | {(fam, "Q", k) for k in range(NCQ)}
        req |= {(fam, x) for x in ("w1", "w2", "D2-no-interior-plane", "D3-one-interior-plane", "D>w+2-all-zero-planes",
                                   "all-depth-edges-in-the-every-tap-region")}
    req |= {("whole", "fwd-rows"), ("whole", "fwd-vec4"), ("whole", "fwd-scalar")}
    req |= {("class-weights", x) for x in ("one-workgroup", "several-workgroups", "a-workgroup-holds-both-branches",
                                           "branches-split-at-a-workgroup", "bwd-ragged")}
    for fam in ("loss", "epe"):
        req |= {(fam, x) for x in ("fewer-than-one-workgroup", "at-least-one-workgroup", "ragged-last-workgroup", "cap-exact",
                                   "cap-threads-walk-more-than-8")}
    req |= {("loss", "partials<=64"), ("loss", "partials==64"), ("loss", "partials>64"), ("epe", "crop-smaller-than-both"),
            ("epe", "every-table-entry-at-columns-0-and-cw-1")}
    return req


def missing_classes(cases=None):
    have = set()
    for c in (CASES if cases is None else cases).values():
        have |= classes_of(c)
    return sorted(required_classes() - have, key=str)


def case_size(c):
    if isinstance(c, CCase):
        return 2 * math.prod(c)
    if isinstance(c, ACase):
        return math.prod(c[:5])
    if isinstance(c, KCase):
        return c.Co * c.C * 54
    if isinstance(c, XCase):
        return 32 * math.prod(c)
    return c.n if isinstance(c, LCase) else c.B * c.Hp * c.Wp


def smallest_case_per_class():
    best = {}
    for name, c in CASES.items():
        for cl in classes_of(c):
            if cl not in best or case_size(c) < case_size(CASES[best[cl]]):
                best[cl] = name
    return best


# ---- threshold tables -------------------------------------------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _dyadic(name, n, lo, hi, step):
    """n pseudo-random multiples of `step` in [lo, hi)."""
    g = torch.Generator().manual_seed(sum(name.encode()) * 7919 + n % 1000003)
    return torch.randint(int(lo / step), int(hi / step), (n,), generator=g).float() * step


LOSS_GT = (0.125, 0.0, 192.0, 100.0, 0.5, 1.0, 3.375, 59.875, 60.0, 60.125, 64.0, 127.875, 160.0, 191.875, 192.125, 255.875, 80.0, 96.5)


def loss_offsets():
    one, three = _f32(1.0), _f32(3.0)
    pos = torch.stack([_f32(2.0 ** -10), 1 - _f32(2.0 ** -10), one, 1 + _f32(2.0 ** -10), three, torch.nextafter(three, _f32(0.0))])
    return torch.cat([_f32([0.0]), pos, -pos])


def loss_table(n):
    """(gt, p1, p2, p3) of n fp32 elements: the threshold table first (and again at the very end where n allows, under the threads
    of the last trip), pseudo-random dyadic values between.  Ground truth: multiples of 1/8 below 256, exact 0 and exact 192
    among them.  Predictions gt + o with o in {0, +-2^-10, +-(1 - 2^-10), +-1, +-(1 + 2^-10), +-3, +-nextafter(3, 0)}, and, for the
    5 % rule of the last head, gt +- o for o = fl(0.05f * gt) and its two neighbours, and the fp32 neighbours of fl(gt +- fl(0.05f * gt))
    (gt + 0.05f * gt has more than 24 bits, so these are the nearest differences fp32 has on either side of the threshold)."""
    offs = loss_offsets()
    gts, o3 = [], []
    for g in LOSS_GT:
        g32 = _f32(g)
        t = _f32(0.05) * g32
        cand = [g32 + o for o in offs]
        for s in (1.0, -1.0):
            for tt in (t, torch.nextafter(t, _f32(math.inf)), torch.nextafter(t, _f32(0.0))):
                cand.append(g32 + s * tt)
            centre = g32 + s * t
            cand += [torch.nextafter(centre, _f32(math.inf)), torch.nextafter(centre, _f32(-math.inf))]
        gts += [g32] * len(cand)
        o3 += cand
    tg, t3 = torch.stack(gts), torch.stack(o3)
    m = tg.numel()
    # the other two heads: the same table, the offsets rotated against the ground truth
    blk = m // len(LOSS_GT)
    t1 = tg + (t3 - tg).view(-1, blk).roll(5, 1).reshape(-1)
    t2 = tg + (t3 - tg).view(-1, blk).roll(11, 1).reshape(-1)
    gt = _dyadic("loss.gt", n, 0, 256, 0.125)
    ps = [gt + _dyadic("loss.o%d" % k, n, -4, 4, 2.0 ** -10) for k in range(3)]
    gt[::13] = 0.0                                                            # a share of pixels outside the mask
    k = min(m, n)
    gt[:k] = tg[:k]
    for p, t in zip(ps, (t1, t2, t3)):
        p[:k] = t[:k]
    if n >= 2 * m:
        gt[-m:] = tg
        for p, t in zip(ps, (t1, t2, t3)):
            p[-m:] = t
    return gt, ps[0], ps[1], ps[2]


def loss_reference(gt, ps, gup, maxdisp=MAXDISP, weights=(0.5, 0.7, 1.0)):
    """fp64 over the mask the fp32 statements select: {loss, m1, m2, m3, epe, count, good, g1, g2, g3} (gradients for an upstream
    gradient `gup` on the loss).  The fp32 decisions -- mask, the two error tests -- are O.train_loss's / O.kitti_metrics's."""
    mask = (gt < maxdisp) & (gt > 0)
    err = torch.abs(ps[2][mask] - gt[mask])                                   # fp32, exact on the table
    good = int(((err < 3) | (err < 0.05 * gt[mask])).sum())
    cnt = int(mask.sum())
    g64 = gt.double()
    out = {"count": cnt, "good": good}
    loss = 0.0
    for k, (p, wk) in enumerate(zip(ps, weights)):
        e = (p.double() - g64)[mask]
        a = e.abs()
        mk = torch.where(a < 1, 0.5 * e * e, a - 0.5).sum() / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)
        out["m%d" % (k + 1)] = mk
        loss = loss + float(_f32(wk)) * mk
        out["g%d" % (k + 1)] = torch.where(mask, gup * float(_f32(wk)) / max(cnt, 1) * (p.double() - g64).clamp(-1, 1), torch.zeros((), dtype=torch.float64))
    out["loss"] = loss
    out["epe"] = err.double().sum() / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)
    return out, mask


EPE_KINDS = 7


def epe_table(c):
    """(pred [B,Hp,Wp], gt [B,Hg,Wg]) fp32.  Inside the crop, columns 0 and cw - 1 and every third pixel elsewhere hold the table:
    d in {-1/8, 0, x, nextafter(x, +inf), nextafter(x, -inf), 192, nextafter(192, 0)} for the pixel's column x, the kind cycling with
    the row; everything else is a pseudo-random multiple of 1/8 in [-8, 260).  pred = d + o, o a multiple of 1/8 (0 where d is
    not one itself: the neighbours of x and of 192), so pred - d is exact."""
    B, Hp, Wp, Hg, Wg, ch, cw = c
    gt = _dyadic("epe.gt", B * Hg * Wg, -8, 260, 0.125).view(B, Hg, Wg)
    x = torch.arange(Wg).view(1, 1, Wg).expand(B, Hg, Wg)
    y = torch.arange(Hg).view(1, Hg, 1).expand(B, Hg, Wg)
    b = torch.arange(B).view(B, 1, 1).expand(B, Hg, Wg)
    xf = x.float()
    inf = torch.full_like(xf, math.inf)
    kinds = torch.stack([torch.full_like(xf, -0.125), torch.zeros_like(xf), xf, torch.nextafter(xf, inf), torch.nextafter(xf, -inf),
                         torch.full_like(xf, 192.0), torch.full_like(xf, float(torch.nextafter(_f32(192.0), _f32(0.0))))], 0)
    kind = (y + b + x // 3) % EPE_KINDS
    table = torch.gather(kinds, 0, kind.unsqueeze(0))[0]
    use = ((x == 0) | (x == cw - 1) | ((y * cw + x) % 3 == 0)) & (x < cw) & (y < ch)
    gt = torch.where(use, table, gt)
    o = _dyadic("epe.o", B * Hg * Wg, -6, 6, 0.125).view(B, Hg, Wg)
    o = torch.where(gt * 8 != (gt * 8).round(), torch.zeros_like(o), o)
    pred = _dyadic("epe.pred", B * Hp * Wp, -8, 260, 0.125).view(B, Hp, Wp)
    pred[:, :ch, :cw] = (gt + o)[:, :ch, :cw]
    return pred, gt


def epe_reference(pred, gt, ch, cw, maxdisp=MAXDISP):
    """O.sceneflow_eval_epe (test.py:69-94) restated to accept a crop: the three masks in fp32 as the reference takes them, then
    (means [3] in fp64 over those masks, counts [3])."""
    d = gt[:, :ch, :cw]
    local = torch.arange(cw).repeat(d.shape[0], d.shape[1], 1).view_as(d).float()
    mask_non = (d < maxdisp) & (d >= 0) & ((local - d) >= 0)
    mask_true = (d < maxdisp) & (d > 0) & ((local - d) >= 0)
    mask = (d < maxdisp) & (d >= 0)
    o = pred[:, :ch, :cw]
    err = torch.abs(o - d)                                                     # fp32, exact on the table
    masks = (mask, mask_non, mask_true)
    means = [err[m].double().sum() / int(m.sum()) if int(m.sum()) else torch.tensor(float("nan"), dtype=torch.float64) for m in masks]
    return torch.stack(means), [int(m.sum()) for m in masks], err, masks


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(src, pattern, what):
    m = re.findall(pattern, src, re.M)
    assert len(m) == 1, f"{what}: {len(m)} matches of {pattern!r}"
    return m[0]


def test_concat_constants_are_those_of_the_source():
    src = _source("costvol.hip")
    assert int(_one(src, r"^constexpr int SEG = (\d+);", "SEG")) == SEG
    assert int(_one(src, r"^constexpr int THREADS = (\d+);", "THREADS")) == THREADS and SEG == 4 * THREADS
    assert src.count("const int dpad = ((D + 3) / 4 + 1) * 4;") == 1 and [dpad(D) for D in (1, 4, 5, 13)] == [8, 8, 12, 20]
    assert src.count("if (w % 4 == 0 && (long long)B * C <= 65535) {") == 2 and GRID_Y_MAX == 65535
    assert src.count("dim3 grid((hw + SEG - 1) / SEG, B * C);") == 2
    assert src.count("(dpad + SEG) * sizeof(float)") == 1 and src.count("if (f >= hw) return;") == 2
    assert concat_path(1, 65535, 4) == "v4" and concat_path(1, 65536, 4) == "scalar" and concat_path(1, 3, 13) == "scalar"


def test_assembly_constants_are_those_of_the_source():
    src = _source("costvol_conv.hip")
    assert _one(src, r"^constexpr int NCP = (\d+), NCQ = (\d+);", "classes") == (str(NCP), str(NCQ))
    assert src.count("const size_t lds = (size_t)(NCP * w + NCQ * (w + 2)) * sizeof(float);") == 1
    assert src.count("const size_t lds = (size_t)D * w * sizeof(float);") == 1
    assert src.count("lds <= 64 * 1024") == 2 and LDS_MAX == 64 * 1024
    assert src.count("const bool aligned = (reinterpret_cast<size_t>(P) | reinterpret_cast<size_t>(y)) % 16 == 0;") == 1
    assert src.count("if (w % 4 == 0 && aligned && lds <= 64 * 1024 && rows <= 0x7fffffffLL) {") == 1
    assert src.count("if (w % 4 == 0 && reinterpret_cast<size_t>(gy) % 16 == 0 && lds <= 64 * 1024 && rows <= 0x7fffffffLL) {") == 1
    assert src.count("    if (w % 4 == 0) {\n        const long long nv = n / 4;") == 1
    assert src.count("const int nP = 15 * Co * C * 9, nQ = 6 * Co * C * 15;") == 1
    assert src.count("const long long n = (long long)Co * C * (15 * 9 + 6 * 15);") == 1
    # the class rules are stated once (cv_fwd_value, cv_ref_sums, cv_tgt_sums) and called by the element-wise and the row-staged kernels
    assert src.count("delta < 3") == 1 and src.count("x == w - 1") == 2 and src.count("+= 256") == 6
    assert src.count("const int hi = da < D - 2 ? da : D - 2;") == 1 and src.count("if (d == 0) { if (rb) firstr += v; else first += v; }") == 1
    assert src.count("cv_fwd_value(d, x0 + k, e, w, ") == 2 and src.count("cv_ref_sums(x, D, ") == 2 and src.count("cv_tgt_sums(j, D, w, ") == 2
    # the gates at the widths of the case table: 776 is the widest row set that fits, 780 the first that does not; 64 x 256 fits exactly
    assert fwd_lds_bytes(776) == 65232 and fwd_lds_bytes(780) == 65568 and fwd_lds_bytes(776) == (21 * 776 + 12) * 4
    assert bwd_lds_bytes(64, 256) == LDS_MAX and bwd_lds_bytes(64, 260) > LDS_MAX
    assert [assemble_fwd_path(w, a) for w, a in ((776, True), (780, True), (776, False), (5, True))] == ["rows", "vec4", "vec4", "scalar"]
    assert [assemble_bwd_path(64, w, a) for w, a in ((256, True), (260, True), (256, False))] == ["rows", "elementwise", "elementwise"]
    assert assemble_bwd_path(3, 5, True) == "elementwise"


def test_reduction_constants_are_those_of_the_sources():
    loss, ev, prep = _source("loss.hip"), _source("eval.hip"), _source("frame_io.h")
    assert int(_one(loss, r"^constexpr int LT = (\d+);", "LT")) == LT and int(_one(ev, r"^constexpr int ET = (\d+);", "ET")) == ET
    assert int(_one(loss, r"^constexpr int LOSS_MAX_BLOCKS = (\d+);", "cap")) == MAX_BLOCKS
    assert int(_one(ev, r"^constexpr int EVAL_MAX_BLOCKS = (\d+);", "cap")) == MAX_BLOCKS
    assert loss.count("long long b = (n + LT * 8 - 1) / (LT * 8);") == 1 and ev.count("long long b = (n + ET * 8 - 1) / (ET * 8);") == 1
    assert PER_THREAD == 8
    assert loss.count("for (int b = threadIdx.x; b < nblocks; b += 64)") == 1 and loss.count("threadIdx.x >= 64") == 1 and FINAL_LANES == 64
    assert int(_one(ev, r"^constexpr int U16_MAXB = (\d+);", "u16 chunk")) == CHUNK
    assert int(_one(prep, r"^constexpr int FP_MAXB = (\d+);", "frame chunk")) == CHUNK
    assert [reduce_blocks(n) for n in (1, 2048, 2049, 64 * 2048, 64 * 2048 + 5, 1024 * 2048, 1024 * 2048 + 2049)] == [1, 1, 2, 64, 65, 1024, 1024]
    # the decisions the threshold tables aim at, as the kernels write them
    assert loss.count("if (g < maxdisp && g > 0.f) {") == 1 and loss.count("a < 1.f ? 0.5f * d * d : a - 0.5f") == 1
    assert loss.count("(a3 < 3.f || a3 < 0.05f * g)") == 1 and loss.count("fminf(fmaxf(") == 3
    assert ev.count("const bool m = d < maxdisp && d >= 0.f;") == 1 and ev.count("((float)x - d) >= 0.f") == 1 and ev.count("d > 0.f") == 1


def test_class_functions_restate_the_kernels():
    # the class of every (d, x) through the vectorised index equals the scalar restatement; classes 9 and 12 cannot occur
    seen_p, seen_q = set(), set()
    for w in (1, 2, 3, 4, 5, 7, 8, 12):
        for D in (2, 3, 4, 5, 9):
            cp, cq, j, valid = class_index(D, w)
            for d in range(D):
                for x in range(w):
                    k = classP(d, x, D)
                    assert bool(valid[d, x]) == (k is not None)
                    if k is not None:
                        assert int(cp[d, x]) == k and int(cq[d, x]) == classQ(d, x, D, w) and int(j[d, x]) == x - d + 2
            P, Q = classes_touched(w, D)
            seen_p |= P
            seen_q |= Q
    assert seen_p == set(range(NCP)) - set(UNREACHABLE_P) and len(seen_p) == 13 and seen_q == set(range(NCQ))
    # 9 and 12 are (d - x = 1 or 2, first plane): d = 0 would need x < 0
    assert [(k // 3 - 2, k % 3) for k in UNREACHABLE_P] == [(1, 0), (2, 0)]
    assert classes_touched(1, 2) == ({6, 11}, {1, 5}) and classes_touched(4, 2)[0] == {0, 3, 6, 2, 5, 8, 11}


GRID = [(w, D, h) for w in (1, 2, 3, 4, 5, 7, 8, 12) for D in (2, 3, 4, 5, 9) for h in (1, 3)]


def test_collapsed_closed_form_equals_conv3d_of_the_volume_in_fp64():
    worst = 0.0
    for w, D, h in GRID:
        B, C, Co = (2, 3, 2) if h == 3 else (1, 2, 3)
        L, R = seeded(f"cg.L{w}.{D}", B, C, h, w).double(), seeded(f"cg.R{w}.{D}", B, C, h, w).double()
        W = seeded(f"cg.W{w}.{D}", Co, 2 * C, 3, 3, 3).double()
        ref = F.conv3d(O.cost_volume(L, R, D), W, None, 1, 1)
        got = collapsed_t(L, R, W, D)
        assert torch.equal(cost_volume_t(L, R, D), O.cost_volume(L, R, D))
        gap = float((got - ref).abs().max()) / float(ref.abs().max())
        worst = max(worst, gap)
        assert gap <= 1e-12, (w, D, h, gap)
        # the 2-D convolutions written as sums over taps are F.conv2d
        wP, wQ = class_weights_t(W)
        assert float((conv2d_taps(L, wP, 1, 1) - F.conv2d(L, wP, None, 1, 1)).abs().max()) <= 1e-12
        assert float((conv2d_taps(R, wQ, 4, 2) - F.conv2d(F.pad(R, (2, 0)), wQ, None, 1, (1, 2))).abs().max()) <= 1e-12
    print(f"collapsed_t vs conv3d(cost_volume), fp64, {len(GRID)} shapes: worst {worst:.2e} of scale")


def test_every_path_class_has_a_case():
    print("missing_classes():", missing_classes())
    assert missing_classes() == []
    for name in ("cv_grid_limit_scalar", "cv_grid_limit_v4", "cv_two_segments", "as_w780", "as_d64_w260", "as_w776", "as_w1",
                 "cw_32x32", "cc_w780", "loss_n%d" % (64 * 2048), "loss_n%d" % (1024 * 2048 + 2049), "epe_tiny"):   # (the check can fail)
        assert missing_classes({k: v for k, v in CASES.items() if k != name}) != [], name
    best = smallest_case_per_class()
    assert set(best) >= required_classes()
    for cl in sorted(best, key=str):
        print("  %-70s %s %s" % (cl, best[cl], tuple(CASES[best[cl]])))
    assert best[("concat", "v4", "single-thread")] == "cv_one_thread" and best[("asm-fwd", "vec4-lds")] == "as_w780"
    assert best[("asm-bwd", "elementwise-lds")] == "as_d64_w260" and best[("whole", "w1")] == "cc_w1"
    # the issue's shapes are in the table
    for shape in ((1, 2, 1, 4, 2), (1, 3, 5, 12, 7), (2, 2, 90, 12, 5), (1, 2, 3, 8, 13), (1, 1, 2, 1028, 6), (1, 3, 7, 13, 5), (1, 2, 2, 1, 3),
                  (1, 65536, 1, 4, 2), (1, 65535, 1, 4, 2)):
        assert CCase(*shape) in CONCAT.values()
    for shape in ((1, 1, 2, 1, 776), (1, 1, 2, 1, 780), (1, 1, 64, 1, 256), (1, 1, 64, 1, 260)):
        assert ACase(*shape, False) in ASSEMBLY.values() and ACase(*shape, True) in ASSEMBLY.values()
    assert {c.w for c in ASSEMBLY.values()} >= {1, 2, 3, 5, 4, 8} and {c.D for c in ASSEMBLY.values()} >= {2, 3, 4}
    assert any(c.D == c.w + 4 for c in ASSEMBLY.values()) and any(c.w == c.D + 4 for c in ASSEMBLY.values())
    assert {tuple(c) for c in WHOLE.values()} == {(1, 1, 1, 2), (1, 2, 2, 3), (2, 3, 9, 5), (1, 2, 12, 16), (1, 1, 780, 2)}
    assert {tuple(c) for c in WEIGHTS.values()} >= {(1, 1), (8, 12), (32, 32)}
    assert all(case_size(c) * 4 <= 10e6 or isinstance(c, (LCase, ECase)) for c in CASES.values())


@pytest.mark.parametrize("n", [c.n for c in LOSS.values() if c.n <= 64 * 2048 + 5])
def test_loss_table_differences_are_exact(n):
    gt, p1, p2, p3 = loss_table(n)
    assert gt.dtype == torch.float32 and gt.numel() == n
    for p in (p1, p2, p3):
        assert torch.equal((p - gt).double(), p.double() - gt.double())
    assert torch.equal(gt * 8, (gt * 8).round()) and float(gt.max()) < 256
    if n < 2049:
        return
    # every boundary is met exactly
    e3, offs = p3 - gt, loss_offsets()
    inm = (gt < MAXDISP) & (gt > 0)
    assert bool((gt == 0).any()) and bool((gt == 192).any()) and bool((gt > 192).any())
    for o in offs:
        assert bool(((e3 == o) & inm).any()), float(o)
        assert bool((((p1 - gt) == o) & inm).any()) and bool((((p2 - gt) == o) & inm).any())
    t = 0.05 * gt
    a3 = e3.abs()
    big = inm & (a3 >= 3)
    assert bool((big & (a3 < t)).any()) and bool((big & (a3 >= t)).any())
    # ... as closely as fp32 allows: within 2 ulp of the prediction on both sides
    ulp = torch.nextafter(p3.abs(), torch.full_like(p3, math.inf)) - p3.abs()
    assert bool((big & (a3 < t) & (t - a3 <= 2 * ulp)).any()) and bool((big & (a3 >= t) & (a3 - t <= 2 * ulp)).any())
    ref, mask = loss_reference(gt, (p1, p2, p3), 1.5)
    assert 0 < ref["good"] < ref["count"] < n and torch.equal(mask, inm)
    # the fp32 statements of the oracle select the same pixels
    epe, err3 = O.kitti_metrics(p3, gt)
    assert abs(float(err3) - (100 - 100 * ref["good"] / ref["count"])) < 1e-3 and abs(float(epe) - float(ref["epe"])) < 1e-4
    assert abs(float(O.train_loss([p.unsqueeze(0).unsqueeze(0) for p in (p1, p2, p3)], gt.unsqueeze(0))) - float(ref["loss"])) < 1e-4


@pytest.mark.parametrize("name", ["epe_tiny", "epe_one_wg", "epe_two_wgs", "epe_many"])
def test_epe_table_differences_are_exact(name):
    c = EPE[name]
    pred, gt = epe_table(c)
    d, o = gt[:, :c.ch, :c.cw], pred[:, :c.ch, :c.cw]
    local = torch.arange(c.cw).float().view(1, 1, -1).expand_as(d)
    assert torch.equal((o - d).double(), o.double() - d.double())
    # x - d: exact wherever it is near its decision (|x - d| < 1; far from it, 680 - nextafter(192, 0) has 25 bits), same sign everywhere
    xd32, xd64 = (local - d).double(), local.double() - d.double()
    assert torch.equal(xd32[xd64.abs() < 1], xd64[xd64.abs() < 1]) and torch.equal(xd32 >= 0, xd64 >= 0)
    means, counts, err, masks = epe_reference(pred, gt, c.ch, c.cw)
    assert counts[0] >= counts[1] >= counts[2]
    if c.ch >= EPE_KINDS:
        assert counts[0] > counts[1] > counts[2] > 0
        for col in (0, c.cw - 1):
            dc, xc = d[..., col], float(col)
            nxt = float(torch.nextafter(_f32(xc), _f32(math.inf))), float(torch.nextafter(_f32(xc), _f32(-math.inf)))
            for v in (-0.125, 0.0, xc, nxt[0], nxt[1], 192.0, float(torch.nextafter(_f32(192.0), _f32(0.0)))):
                assert bool((dc == v).any()), (col, v)


def test_epe_restatement_is_the_oracle_at_its_own_crop():
    c = ECase(1, 545, 970, 541, 961, 540, 960)
    pred, gt = epe_table(c)
    means, counts, _, _ = epe_reference(pred, gt, 540, 960)
    want = O.sceneflow_eval_epe(pred, gt)
    assert all(abs(float(m) - v) <= 1e-5 * abs(v) for m, v in zip(means, want))
