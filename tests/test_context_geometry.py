"""The path table of tests/test_hip_context_fp64.py, checked without a GPU: its restatement of the host-side dispatch of the
context-mapping kernels uses the constants of csrc/ecm_weights.hip, ecm_weights_bwd.hip, ecm_nbr.h, heads.hip and variants.hip as
they stand in the sources (a retune must not silently move the cases off the paths they were chosen for), every path class has a
case, every weights case keeps its share of pixels at a LeakyReLU kink under the cap, and the closed forms that serve as second
fp32 evaluations equal the oracle in fp64."""
import os
import re

import pytest

import test_hip_context_fp64 as T
from conftest import ROOT

CSRC = os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(src, pattern, what):
    m = re.findall(pattern, src, re.M)
    assert len(m) == 1, f"{what}: {len(m)} matches of {pattern!r}"
    return m[0]


def _table(body, fn, n):
    m = re.search(r"int " + fn + r"\(int n\) \{ (?:constexpr int t\[" + str(n) + r"\] = \{([-\d, ]+)\}; return t\[n\];|return (\d+);) \}", body)
    assert m, fn
    return tuple(int(v) for v in m.group(1).split(",")) if m.group(1) else (int(m.group(2)),) * n


def test_weight_kernel_constants_are_those_of_the_sources():
    fwd, bwd = _source("ecm_weights.hip"), _source("ecm_weights_bwd.hip")
    assert _one(fwd, r"^constexpr int CF = (\d+);", "forward CF") == str(T.CF)
    assert _one(fwd, r"^constexpr int TX = (\d+), TY = (\d+);", "forward tile") == (str(T.TX), str(T.TY))
    assert _one(bwd, r"^constexpr int CF = (\d+), TX = (\d+), TY = (\d+);", "backward tile") == (str(T.CF), str(T.TX), str(T.TY))
    assert _one(bwd, r"^constexpr int NCXMAX = (TX / 4 \+ 2), NCY = 3;", "NCXMAX") and T.NCXMAX == T.TX // 4 + 2
    assert int(_one(bwd, r"^constexpr int UST = (\d+);", "UST")) == T.UST
    assert int(_one(bwd, r"PB_W3 = \d+, PB_N = (\d+);", "PB_N")) == T.PB_N
    # plan(): tiles of TX columns and TY rows, at most 512 workgroups, 128 cells per workgroup of the cells kernel
    assert _one(bwd, r"p\.tiles_x = \(w \* s \+ TX - 1\) / (TX);", "tiles_x") and _one(bwd, r"rbs = \(long long\)h \* s / (TY);", "rbs")
    assert _one(bwd, r"p\.nB = \(int\)\(p\.ntiles < (\d+) \? p\.ntiles : (\d+)\);", "nB") == (str(T.MAX_WORKERS),) * 2
    assert int(_one(bwd, r"p\.nC = \(int\)\(\(\(long long\)B \* h \* w \+ 127\) / (\d+)\);", "nC")) == T.CELL_BLOCK
    assert int(_one(bwd, r"const long long i = \(long long\)blockIdx\.x \* (\d+) \+ threadIdx\.x;\n    const bool valid", "cells block")) == T.CELL_BLOCK
    assert _one(bwd, r"const int lpc = (4 \* s);", "lanes per cell") and _one(bwd, r"const int hw = h \* w, rpc = (s / TY),", "rpc")
    # the reduce kernel: 8 lane groups, an unrolled loop of 4 strides, a tail loop -- the one statement of partial_sum.h, which
    # the kernel calls around its source table
    psum = _source("partial_sum.h")
    assert _one(psum, r"for \(; (p \+ 24 < n; p \+= 32)\)", "unrolled loop") and _one(psum, r"for \(; (p < n; p \+= 8)\)", "tail loop")
    assert _one(psum, r"(return \(s0 \+ s1\) \+ \(s2 \+ s3\);)", "pairing") and _one(psum, r"(__shared__ float sm\[8\]\[32\];)", "tail")
    assert _one(bwd, r"(s = partial_group_sum\(src, stride, n, grp\);)", "the call") and _one(bwd, r"(partial_tail\(s, o, grp, k < 2760, gW \+ k\);)", "tail")
    all_src = "".join(_source(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h")))
    assert all_src.count("p + 24 <") == 1 and all_src.count("sm[8][32]") == 1          # one eight-group partial sum in the library
    # the backward's gate, in the size query and in the entry point
    gate = "(s != 4 && s != 8 && s != 16)"
    assert bwd.count(gate) == 2 and T.BWD_SCALES == (4, 8, 16)
    assert fwd.count("if (variant == 0 && s != 4) return ECM_EUNSUP;") == 1 and "s % 2 != 0" in fwd
    # the forward's cell window and its LDS bound
    assert "ncy = (Y0 + TY - 1) / s - Y0 / s + 3, ncx = (X0 + TX - 1) / s - X0 / s + 3;" in fwd
    assert "const int ncy = (TY - 1) / s + 4, ncx = (TX - 1) / s + 4;" in fwd
    assert "dim3 grid((W + TX - 1) / TX, (H + TY - 1) / TY, B);" in fwd


def test_neighbour_tables_are_those_of_the_source():
    src = _source("ecm_nbr.h")
    for var, nbr in T.NBR.items():
        body = re.search(r"template <> struct Nbr<%d> \{(.*?)\n\};" % var, src, re.S).group(1)
        n = int(re.search(r"static constexpr int N = (\d+);", body).group(1))
        assert n == len(nbr)
        got = tuple(zip(_table(body, "dy", n), _table(body, "dx", n), _table(body, "tab", n)))
        assert got == nbr, var
        assert ("PAD = -100.f" in body) == (var == 0) and ("FINAL_ACT = true, TIMES_LOGIT = true" in body) == (var != 0)
    # the oracle's tables are the same ones
    assert T.NBR[0] == T.O.EIGHT_NEIGHBOURS and T.NBR[1] == T.O.SIX_LEFT and T.NBR[2] == T.O.SIX_RIGHT


def test_head_launches_are_those_of_the_sources():
    heads, var = _source("heads.hip"), _source("variants.hip")
    per_element = "dim3 grid((unsigned)((n + 255) / 256)), block(256);"
    assert heads.count(per_element) == 4 and var.count(per_element) == 3 and T.THREADS == 256
    # aggregate9_bwd_d: one wave per LR cell, four per workgroup
    assert "dim3 grid2((unsigned)((cells + 3) / 4));" in heads and "blockIdx.x * 4 + (threadIdx.x >> 6);" in heads
    assert "for (int j = lane; j < 9 * ss; j += 64)" in heads
    # volume_mapping_bwd: one wave per image row, four per workgroup, chunks of 64 columns, a [3][W] LDS row per wave
    assert "dim3 grid((unsigned)(((long long)B * H + 3) / 4)), block(256);" in var and "blockIdx.x * 4 + wave;" in var
    assert "for (int X0 = 0; X0 < W; X0 += 64)" in var and "(size_t)4 * 3 * W * sizeof(float)" in var and "lds > 160 * 1024" in var
    assert "(s & (s - 1)) != 0 || s > 64" in var and T.ROWS_PER_WG == 4
    assert heads.count("__launch_bounds__(256)") == 6 and var.count("__launch_bounds__(256)") == 7


def test_restated_geometry_on_known_shapes():
    # 576 x 960 at scale 4: 15 x 144 tiles on 512 workgroups; the issue's two walk examples: 520 tiles each
    p = T.bwd_plan(1, 144, 240, 4)
    assert (p["tiles_x"], p["rbs"], p["ntiles"], p["nB"], p["nC"], p["rpc"], p["lpc"]) == (15, 144, 2160, 512, 270, 1, 16)
    assert T.bwd_plan(2, 20, 208, 4)["ntiles"] == 520 and T.bwd_plan(1, 13, 40, 16)["ntiles"] == 520
    assert T.bwd_plan(1, 4, 4, 16) == dict(tiles_x=1, rbs=16, ntiles=16, nB=16, nC=1, rpc=4, lpc=64)
    grid, win = T.fwd_geom(1, 3, 37, 2)
    assert grid == (2, 2, 1) and win[0, 0] == (-1, -1, 4, 34) and win[1, 1] == (1, 31, 4, 34)       # a 4-row tile over two cell rows
    grid, win = T.fwd_geom(1, 2, 12, 6)
    assert grid == (2, 3, 1) and win[1, 1][:2] == (-1, 9) and 64 % 6 == 4                             # rows 4..7 span cells 0 and 1
    assert [T.reduce_bucket(n) for n in (1, 7, 8, 24, 25, 30, 32, 56, 64, 512)] == \
        ["idle-groups"] * 2 + ["tail-loop-only"] * 2 + ["unrolled-edge"] * 2 + ["unrolled", "unrolled-edge", "unrolled", "unrolled"]
    assert T.unsampled_planes(T.TRILINEAR["tl_down"]) == [0, 3, 4, 7] and T.unsampled_planes(T.TRILINEAR["tl_up4"]) == []
    assert T.aggregate_grids(1, 3, 5, 2) == (1, 4) and T.volume_grids(1, 3, 19, 4) == (4, 3, 2) and T.trilinear_grid(2, 8, 11) == 1


def test_every_path_class_has_a_case():
    assert T.missing_classes() == []
    for name in ("w0s4_walk", "w2s16_ragged16", "w1s8_ragged_30", "w2s2_fwd", "tl_down", "vm_s2", "ag_s2", "sa_d1"):   # (the check can fail)
        assert T.missing_classes({k: v for k, v in T.CASES.items() if k != name}) != [], name
    # a 4-row tile at s = 2 counts only where both of its cell rows are inside the image
    assert T.missing_classes({**T.CASES, "w2s2_fwd": T.WCase(2, 2, 1, 35, 2, False)}) == [("fwd", 2, "s2-tile-spans-two-cell-rows")]
    best = T.smallest_case_per_class()
    assert set(best) >= T.required_classes()
    assert best[("bwd", "v0", "one-and-two-tiles-per-workgroup")] == "w0s4_walk" and best[("reduce", "nB", "idle-groups")].endswith("_w1")


@pytest.mark.parametrize("name", sorted(k for k, c in T.WEIGHTS.items() if c.grads))
def test_kink_share_is_under_the_cap(name):
    keep, share = T.kink(name)
    c = T.CASES[name]
    assert keep.shape == (c.B, 1, c.h * c.s, c.w * c.s) and abs((1 - keep).mean().item() - share) < 1e-6
    assert share <= T.KINK_SHARE, f"{name}: {share:.3%} of the pixels lie within {T.KINK_EPS} of a LeakyReLU kink"


def test_closed_forms_equal_the_oracle_in_fp64():
    gaps = T.closed_form_gaps()
    assert len(gaps) >= 40
    bad = {k: v for k, v in gaps.items() if not v <= 1e-12}
    assert not bad, bad
