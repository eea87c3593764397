"""The 2-D convolution path table of tests/test_hip_conv2d_fp64.py, checked without a GPU: its restatement of the host-side
dispatch uses the constants, thresholds and template arguments of csrc/conv2d_kernel.h, fp32_conv_stage.h, the seven conv2d_case_*.hip,
conv3d_wgrad.hip (2-D part), conv_wino.hip (KD 1), deconv3d.hip (KD 1), conv2d_c1.hip and ops.py as they stand in the sources (a
retune must not silently move the cases off the paths they were chosen for), every path class has a case, the restatements that
enter the unit are the convolution itself, and the operands of the conv2d_c1_relu cases leave at most 0.1 % of the outputs within
1e-5 of the ReLU's kink."""
import os
import re

import pytest
import torch

import test_hip_conv2d_fp64 as T
from conftest import ROOT
from test_conv3d_geometry import _body, _constexpr, _ints, _read, stage_constants_exist_once

PKG = os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd")


def test_conv2d_mfma_dispatch_is_that_of_the_source():
    src = _read("csrc", "conv2d_kernel.h")
    assert stage_constants_exist_once() == T.TW
    assert "static constexpr int TH = 4 * NT;" in src
    plan = _body(src, "inline C2Plan c2_plan(")
    assert "p.cot = Co <= 32 ? 1 : Co <= 64 ? 2 : (kh * kw != 1 && Co % 96 == 0 && Co % 128 != 0) ? 3 : 4;" in plan
    assert "p.cic = (kh * kw == 1) ? 8 : 4;" in plan
    assert "p.groups = (Co + p.cot * 32 - 1) / (p.cot * 32);" in plan and "p.cip = (Ci + p.cic - 1) / p.cic * p.cic;" in plan
    # the default of c2_min_blocks(), and that the environment variable is read once into a static
    mb = _body(src, "inline int c2_min_blocks(")
    assert _ints(mb, r'static const int v = \[\] \{ const char\* e = getenv\("ECM_C2_MIN_BLOCKS"\); const int x = e \? atoi\(e\) : 0; '
                 r"return x > 0 \? x : (\d+); \}\(\);", "c2_min_blocks") == (T.C2_MIN_BLOCKS,) == (1536,)
    nt = _body(src, "inline int c2_nt(")
    assert "for (int nt = max_nt; nt > 1; nt >>= 1)" in nt
    assert "if (cols_x_groups * ((Ho + 4 * nt - 1) / (4 * nt)) >= c2_min_blocks()) return nt;" in nt and "return 1;" in nt
    disp = _body(src, "int dispatch_c2(")
    assert "const long long cg = (long long)B * ((Wo + TW - 1) / TW) * p.groups;" in disp
    for cot, n in T.C2_NT_K11.items():
        assert "if constexpr ((COTS & %d) != 0) if (p.cot == %d) { C2_GO(%d, %d, 8); }" % (1 << cot, cot, cot, n) in disp
    b, s = T.C2_NT[1]
    assert ("if constexpr ((COTS & 2) != 0) if (p.cot == 1) { if constexpr (STRIDE == 1) { if (c2_nt(cg, Ho, %d) >= %d) "
            "{ C2_GO(1, %d, 4); } } C2_GO(1, %d, 4); }" % (b, b, b, s)) in disp
    for cot in (2, 4):
        b, s = T.C2_NT[cot]
        assert ("if constexpr ((COTS & %d) != 0) if (p.cot == %d) { if (c2_nt(cg, Ho, %d) >= %d) { C2_GO(%d, %d, 4); } C2_GO(%d, %d, 4); }"
                % (1 << cot, cot, b, b, cot, b, cot, s)) in disp
    assert "if constexpr ((COTS & 8) != 0) if (p.cot == 3) { C2_GO(3, %d, 4); }" % T.C2_NT[3][0] in disp and T.C2_NT[3][0] == T.C2_NT[3][1]
    assert disp.count("C2_GO(") == 3 + 2 + 2 + 1 + 2 + 1                # (+ 1: the #define)
    launch = _body(src, "int launch_c2(")
    assert "tiles_h = (Ho + Cfg::TH - 1) / Cfg::TH, tiles_w = (Wo + TW - 1) / TW;" in launch
    assert "(long long)B * tiles_h * tiles_w, (unsigned)groups, 256," in launch           # the co groups are the grid's y extent
    assert "hipLaunchKernelGGL(kern, dim3((unsigned)nblk, ngrp), dim3(nthr), lds, st, args...);" in _read("csrc", "fp32_conv_stage.h")
    assert "int bid = ecm_xcd_tile(blockIdx.x, gridDim.x);" in src and "if (oh >= Ho || ow >= Wo) continue;" in src
    assert "if (co < Co) yp[(size_t)co * HWo] = acc[r][ct][i];" in src


def test_conv2d_cases_are_those_of_the_sources():
    names = {(3, 3, 1, 1): "k33_s1_d1", (3, 3, 1, 2): "k33_s1_d2", (3, 3, 1, 4): "k33_s1_d4", (3, 3, 2, 1): "k33_s2_d1",
             (3, 5, 1, 1): "k35_s1_d1", (1, 1, 1, 1): "k11_s1", (1, 1, 2, 1): "k11_s2"}
    assert set(names) == set(T.C2_COTS)
    files = sorted(f for f in os.listdir(os.path.join(PKG, "csrc")) if re.fullmatch(r"conv2d_case_.*\.hip", f))
    assert files == sorted("conv2d_case_%s.hip" % n for n in names.values())
    top = _read("csrc", "conv2d.hip")
    for case, n in names.items():
        src = _read("csrc", "conv2d_case_%s.hip" % n)
        got = _ints(src, r"return dispatch_c2<(\d+), (\d+), (\d+), (\d+), (\d+)>\(", "dispatch_c2 in " + n)
        assert got == case + (T.C2_COTS[case],)
        assert "C2_CASE(%d, %d, %d, %d, ecm_c2_%s);" % (case + (n,)) in top
    assert top.count("C2_CASE(") == len(names) + 1
    ops = _read("ops.py")
    m = re.search(r"^_C2_CASES = (\{.*?\n.*?\})\n", ops, re.M | re.S)
    assert eval(m.group(1)) == T.ops_c2_cases()                          # a dict literal of tuples and sets
    cot = _body(ops + "\n}\n", "def _cot(Co, kh, kw):")
    assert "    if Co <= 32:\n        return 1\n    if Co <= 64:\n        return 2\n" in cot
    assert "    return 3 if (kh * kw != 1 and Co % 96 == 0 and Co % 128 != 0) else 4\n" in cot
    sup = _body(ops + "\n}\n", "def conv2d_supported(")
    for line in ("    if cots is None or _cot(Co, kh, kw) not in cots:\n        return False\n",
                 "    if stride == 1:\n        return _cot(Ci, kh, kw) in cots", "        return Ci <= 64 and Co % 4 == 0\n",
                 "    return _cot(Ci, 1, 1) in _C2_CASES[(1, 1, 1, 1)]"):
        assert line in sup, line
    for Co in (1, 32, 33, 64, 65, 96, 128, 192, 384, 480):
        for k in ((3, 3), (1, 1), (3, 5)):
            assert T.ops_cot(Co, *k) == T.c2_plan(4, Co, *k)["cot"]
    assert T.conv2d_supported(32, 480, 3, 3, 1, 1) and T.conv2d_supported(32, 192, 3, 5, 1, 1) and T.conv2d_supported(3, 32, 3, 3, 2, 1)
    assert not T.conv2d_supported(64, 64, 3, 5, 1, 1) and not T.conv2d_supported(96, 100, 3, 3, 1, 4) and not T.conv2d_supported(96, 64, 1, 1, 3, 1)


def test_winograd_rule_is_that_of_the_source():
    ops = _read("ops.py")
    assert _ints(ops, r'^WINO2D_MIN_CI = int\(_os\.environ\.get\("ECM_WINO2D_MIN_CI", "(\d+)"\)\)', "WINO2D_MIN_CI") == (T.WINO2D_MIN_CI,)
    assert "same = (kh, kw, stride, dil, pad_top, pad_left) == (3, 3, 1, 1, 1, 1) and (Ho, Wo) == tuple(x.shape[-2:])" in ops
    assert "ctx.wino_f, ctx.wino_b = _wino_ok(x) and same and Ci >= WINO2D_MIN_CI, _wino_ok(x) and same and Co >= WINO2D_MIN_CI" in ops
    assert "            if ctx.wino_same and _wino_ok(x) and WINOGRAD_WGRAD:\n                return _wino_wgrad(x, gy, Co, Ci, 1, w)" in ops
    assert "    vol = x.shape[-1] * x.shape[-2] * (x.shape[-3] if x.dim() == 5 else 1)\n" in ops
    assert "    return WINOGRAD and x.shape[-1] >= 2 and vol * 128 <= 0x80000000\n" in ops
    assert "    pt = dil * (kh - 1) // 2 if pad_top is None else int(pad_top)" in ops
    assert "        Ho = (H + 2 * pt - dil * (kh - 1) - 1) // stride + 1" in ops
    assert "    Qp = conv2d(right, wQ, 1, 1, 1, 4, h, w + 2)" in ops and "    P = conv2d(left, wP, 1, 1, 1, 1, h, w)" in ops
    assert T.geometry(T.CASES["m35_q_small"]) == (1, 4, 6, 13) and T.geometry(T.CASES["m33_p_small"]) == (1, 1, 6, 11)
    src = _read("csrc", "conv_wino.hip")
    assert _ints(src, r"^constexpr int WINO_CIC3 = \d+, WINO_CIC2 = (\d+);", "WINO_CIC2") == (T.WINO_CIC2,)
    assert "if (kd == 1) return launch_wino<%d, %d, %d, WINO_CIC2>(" % T.WINO_INST[:3] in src
    launch = _body(src, "int launch_wino(")
    assert "tiles_d = (D + TD - 1) / TD, tiles_wt = (W + 1) / 2, ntile = ((H + 1) / 2) * tiles_wt;" in launch
    assert _ints(launch, r"const int tblocks = \(ntile \+ (\d+) \* TR - 1\) / \((\d+) \* TR\);", "tile block") == (T.WINO_BLOCK,) * 2
    assert "const int groups = (Co + 31) / 32, nchunks = (Ci + CIC - 1) / CIC;" in launch
    assert T.wino_ok((6, 2)) and not T.wino_ok((6, 1)) and not T.wino_ok((6, 8), False) and not T.wino_ok((4096, 4097))
    assert T.wino_ok((16, 6, 7)) and not T.wino_ok((16, 1024, 1025))


def test_weight_gradient_dispatch_is_that_of_the_source():
    src = _read("csrc", "conv3d_wgrad.hip")
    assert (_constexpr(src, "CT", "conv3d_wgrad.hip"), _constexpr(src, "TWV", "conv3d_wgrad.hip")) == (T.CT, T.TWV)
    # the table of the general 2-D family: one Wg2<KH, KW, S, DL, TH> per instantiation, in wg2_select alone
    sel = _body(src, "int wg2_select(")
    got = {tuple(map(int, m[:4])): int(m[4]) for m in re.findall(r"Wg2<(\d+), (\d+), (\d+), (\d+), (\d+)>", sel)}
    assert got == T.WG2_TH and len(re.findall(r"Wg2<\d", src)) == len(T.WG2_TH) == 7
    assert "template <int KH, int KW, int S, int DL, int TH> using Wg2 = WgCfg<S, 1, TH, 1, KH, KW, DL>;" in src
    assert "Cfg::KH == kh && Cfg::KW == kw && Cfg::S == stride && (dil < 0 || Cfg::DIL == dil);" in sel
    body = _body(src, 'extern "C" int ecm_conv2d_wgrad_ex(')
    assert ("return launch_wgrad<Cfg>(x, gy, gw, static_cast<float*>(scratch), plan<Cfg>(B, Ci, Co, 1, Ho, Wo), B, Ci, Co, 1, H, W,\n"
            "                                 ecm_stream(stream), pad_top, pad_left);") in body
    assert "return wg2_select(kh, kw, stride, dil, [&](auto c) {" in body
    assert "conv3d_wgrad_mfma<Cfg::S, Cfg::TD, Cfg::TH, Cfg::KD, Cfg::KH, Cfg::KW, Cfg::DIL>" in _body(src, "int launch_wgrad(")
    # the query: the row of (kh, kw, stride) at any dilation; outside the table the 3x3 row of the stride (TH 16 | 8)
    q = _body(src, "inline WgPlan wg2_query_plan(")
    assert "p = plan<decltype(c)>(B, Ci, Co, 1, Ho, Wo);" in q
    assert "if (wg2_select(kh, kw, stride, -1, take) != 0) wg2_select(3, 3, stride == 1 ? 1 : 2, -1, take);" in q
    assert (T.WG2_TH[(3, 3, 1, 1)], T.WG2_TH[(3, 3, 2, 1)]) == (16, 8)
    assert len({th for (kh, kw, s, d), th in T.WG2_TH.items() if s == 1}) == len({th for (kh, kw, s, d), th in T.WG2_TH.items() if s == 2}) == 1
    assert _ints(src, r"^constexpr int WG2_MAX_KG = (\d+);", "WG2_MAX_KG") == (4,)
    assert "wg2_query_plan(B, Ci, Co, Ho, Wo, kh, kw, stride).P * WG2_MAX_KG * Co * Ci * kh * kw * (long long)sizeof(float);" in src
    assert "static_assert(Cfg::KD == 3 || Cfg::KG <= WG2_MAX_KG," in _body(src, "int launch_wgrad(")
    workers = _body(src, "WgPlan plan(")
    assert "p.ci_tiles = (Ci + CT - 1) / CT; p.co_tiles = (Co + CT - 1) / CT;" in workers
    assert _ints(workers, r"long long workers = (\d+) \* Cfg::OCC / \(p\.ci_tiles \* p\.co_tiles\);", "workers") == (T.WGRAD_WORKERS,)
    assert "if (workers < 1) workers = 1;" in workers and "if (workers > p.ntiles) workers = p.ntiles;" in workers
    assert src.count("static constexpr int OCC = KD == 3 ? 1 : 2;") == 1 and src.count("KD == 3 ? 1 : 2") == 1 and T.WGRAD_OCC2D == 2
    assert "wg_select<WgCfg<1, 2, 8, 3>, WgCfg<1, %d, %d, %d>>(" % T.WGW_INST in _body(src, "int wgw_select(")
    assert ("p.tiles_d = (Do + Cfg::TD - 1) / Cfg::TD; p.tiles_h = (Ho + Cfg::TH - 1) / Cfg::TH; p.tiles_w = (Wo + TWV - 1) / TWV;"
            in workers)
    assert "true>(B, Ci, Co, D, H, W);" in _body(src, 'extern "C" int ecm_conv_wino_wgrad(')
    ops = _read("ops.py")
    assert '"ecm_conv2d_wgrad_ex",\n                          _p(gy), _p(x), _p(gw), _SCRATCH, B, Co, Ci, Ho, Wo, 3, 3, 2, 1, 1, 1, H, W, _stream())' in ops


def test_deconv_and_c1_constants_are_those_of_the_sources():
    src = _read("csrc", "deconv3d.hip")
    assert stage_constants_exist_once() == T.TW
    assert _ints(src, r"static constexpr int TD = (\d+), TH = (\d+), NTAPS = 9 \* KD;", "DeconvCfg") == (1, T.DECONV_TH)
    for fn, tail in (("ecm_deconv2d_k3s2_fwd", ""), ("ecm_deconv2d_k3s2_bias_fwd", ", true")):
        body = _body(src, 'extern "C" int %s(' % fn)
        assert "if (Co > 32) return launch_deconv<2, %d, 1%s>(" % (T.DECONV_CIC, tail) in body
        assert "    return launch_deconv<1, %d, 1%s>(" % (T.DECONV_CIC, tail) in body
        assert "if (Ci % 4 != 0 || Co < 1 || Co > 64) return ECM_EUNSUP;" in body
        assert "if (Ho > 2 * H || Ho < 2 * H - 1 || Wo > 2 * W || Wo < 2 * W - 1) return ECM_EUNSUP;" in body
    assert "tiles_d = (D + Cfg::TD - 1) / Cfg::TD, tiles_h = (H + Cfg::TH - 1) / Cfg::TH, tiles_w = (W + TW - 1) / TW;" in src
    c1 = _read("csrc", "conv2d_c1.hip")
    assert _ints(c1, r"^constexpr int C1_TX = (\d+), C1_TY = (\d+);", "C1_TX, C1_TY") == (T.C1_TX, T.C1_TY)
    got = {n: _constexpr(c1, n, "conv2d_c1.hip") for n in ("C1_CC", "C1_SUB", "C1_CHUNK")}
    assert got == {n: getattr(T, n) for n in got}
    plan = _body(c1, "inline C1WgPlan c1_wgrad_plan(")                  # read by the scratch query and by the launcher
    assert "p.strips_y = (H + C1_TY * C1_SUB - 1) / (C1_TY * C1_SUB);" in plan and "p.tiles_x = (W + C1_TX - 1) / C1_TX;" in plan
    assert "p.P = (long long)B * p.strips_y * p.tiles_x;" in plan and "p.n = Ci * 9 + 1;" in plan
    assert c1.count("c1_wgrad_plan(B, Ci, H, W);") == 2 and "c1_strips" not in c1
    wg = _body(c1, 'extern "C" int ecm_conv2d_c1_wgrad(')
    assert "dim3((unsigned)p.P)" in wg                                  # one workgroup per strip: the worker count is not capped
    assert c1.count("const int tx = (W + C1_TX - 1) / C1_TX, ty = (H + C1_TY - 1) / C1_TY;") == 2
    cs = _body(c1, 'extern "C" int ecm_channel_sum(')
    assert "const long long chunks = (HW + C1_CHUNK - 1) / C1_CHUNK;" in cs
    assert "if ((HW & 3) == 0 && (reinterpret_cast<size_t>(x) & 15) == 0) {" in c1


def test_restated_dispatch_on_known_shapes():
    """The figures the sources and the issue quote: 4 -> 8 at 4 x 600 x 641 is 1596 blocks of TH 32; the stem at full size
    takes the same tile; 64 -> 128 forward is cot 4 and its data gradient cot 2."""
    g = T.c2_fwd(4, 4, 8, 600, 641, 3, 3, 1, 1)
    assert g["inst"] == (1, 8, 4) and g["TH"] == 32 and g["nblk"] == 4 * 21 * 19 == 1596 and g["ragged"] == (True, True)
    assert T.c2_fwd(3, 4, 8, 600, 641, 3, 3, 1, 1)["inst"] == (1, 4, 4)                 # 1197 blocks of TH 32: below the threshold
    assert T.c2_fwd(4, 3, 32, 576, 960, 3, 3, 1, 1)["inst"] == (1, 8, 4)                # the stem at full size
    assert T.c2_fwd(1, 64, 128, 10, 35, 3, 3, 1, 1)["inst"][0] == 4 and T.c2_fwd(1, 128, 64, 10, 35, 3, 3, 1, 1)["inst"][0] == 2
    g = T.c2_fwd(1, 32, 480, 6, 11, 3, 3, 1, 1)
    assert g["inst"] == (3, 2, 4) and g["groups"] == 5
    g = T.wg2_geom(1, 128, 128, 90, 90, 3, 3, 1, 1)
    assert (g["P"], g["ntiles"]) == (32, 36) and sorted(set(g["runs"])) == [1, 2] and sum(g["runs"]) == 36
    g = T.wg2_geom(2, 40, 72, 100, 100, 3, 3, 1, 1)
    assert (g["P"], g["ntiles"]) == (85, 98) and g["runs"] == [2] * 13 + [1] * 72
    g = T.wg2_geom(2, 64, 96, 41, 120, 3, 3, 2, 1)                              # Deconv2dK3S2Bias.backward at 96 -> 64
    assert (g["P"], g["ntiles"]) == (85, 96)
    g = T.wino_geom(1, 4, 8, 1, 49, 6)
    assert (g["tiles_wt"], g["ntile"], g["tblocks"], g["nchunks"]) == (3, 75, 2, 1)
    assert T.c1_geom(2, 8, 130, 70)["workers"] == 2 * 2 * 2 and T.c1_geom(2, 8, 130, 70)["tiles"] == 2 * 5 * 2
    assert T.chsum_geom(1, 3, 131 * 127) == dict(chunks=2, vec=False)


def test_every_path_class_has_a_case():
    assert T.missing_classes() == []
    reached = {(g["case"], g["inst"]) for c in T.CASES.values() for q, fam, g in T.launches(c) if fam == "c2" and q == "y"}
    assert reached == set(T.all_c2_instantiations())
    wg = {g["kind"] for c in T.CASES.values() for _, fam, g in T.launches(c) if fam == "wg2"}
    assert wg == set(T.WG2_TH)
    assert len(set(T.CASES.values())) == len(T.CASES), "two cases share one specification"
    for name, c in T.CASES.items():                                     # what ops would refuse is no case
        if c.op == "conv" and c.grads == "all":
            assert T.conv2d_supported(c.Ci, c.Co, *c.k, c.stride, c.dil), name
        if c.grads == "none":
            assert c.Ci <= 12, name


def test_the_check_can_fail(monkeypatch):
    """A retuned threshold moves the large-tile cases onto the small tiles, and missing_classes() says so."""
    monkeypatch.setattr(T, "C2_MIN_BLOCKS", 2048)
    missing = T.missing_classes()
    assert any("(1, 8, 4)" in m for m in missing) and any("(2, 4, 4)" in m for m in missing) and any("(4, 2, 4)" in m for m in missing)


def test_restatements_are_the_convolution_in_fp64():
    """The Winograd and the summation-order candidates of the unit evaluate the same operation: the checks of the GPU module, here."""
    for shape in T.RESTATEMENT_SHAPES:
        T.test_winograd2d_restatement_is_the_convolution(shape)
    for shape in T.CHAIN_SHAPES:
        T.test_chain2d_restatement_is_the_convolution(shape)
    x, w = T.seeded("c2.rs.x", 1, 2, 4, 5), T.seeded("c2.rs.w", 3, 2, 3, 3)
    assert T.wino2_fwd(x, w).dtype == torch.float32 and T.wino2_wgrad(x, T.wino2_fwd(x, w)).shape == w.shape


@pytest.mark.parametrize("name", sorted(n for n, c in T.CASES.items() if c.op == "c1"))
def test_relu_boundary_share(name):
    """At most 0.1 % of a conv2d_c1_relu case's outputs lie within 1e-5 of zero before the ReLU (they are left out of the
    comparison), and the bias leaves roughly half of them clamped: a property of the operands alone, in fp64."""
    share, clamped = T.relu_boundary_share(name)
    assert share <= T.RELU_SHARE, (name, share)
    assert 0.3 <= clamped <= 0.7, (name, clamped)
