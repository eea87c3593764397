"""The 3-D convolution path table of tests/test_hip_conv3d_fp64.py, checked without a GPU: its restatement of the host-side
dispatch uses the constants, thresholds and template arguments of csrc/conv3d.hip, fp32_conv_stage.h, conv_wino.hip,
conv3d_wgrad.hip, deconv3d.hip, conv3d_c1.hip and ops.py as they stand in the sources (a retune must not silently move the cases off the paths they were chosen
for), every path class has a case, and the Winograd restatement that enters the unit is the convolution itself."""
import os
import re

import torch

import test_hip_conv3d_fp64 as T
from conftest import ROOT

PKG = os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd")


def _read(*parts):
    with open(os.path.join(PKG, *parts)) as f:
        return f.read()


def _ints(src, pattern, what):
    m = re.findall(pattern, src, re.M)
    assert len(m) == 1, f"{what}: {len(m)} matches"
    return tuple(int(v) for v in (m[0] if isinstance(m[0], tuple) else (m[0],)))


def _constexpr(src, name, what):
    return _ints(src, r"^constexpr int [^;]*\b" + name + r" = (\d+)\b", f"{name} in {what}")[0]


def stage_constants_exist_once():
    """TW and the staging geometry live in fp32_conv_stage.h alone: the three kernels that are built on it define none of them."""
    stage = _read("csrc", "fp32_conv_stage.h")
    users = [_read("csrc", f) for f in ("conv3d.hip", "deconv3d.hip", "conv2d_kernel.h")]
    for u in users:
        assert '#include "fp32_conv_stage.h"' in u
    for pattern in (r"constexpr int TW\b", r"typedef float f32x16\b", r"constexpr int NPOS =", r"constexpr int PP =", r"constexpr int NX =",
                    r"constexpr int NWQ =", r"constexpr int XS_FLOATS =", r"constexpr int WS_FLOATS =", r"constexpr int LDS_BYTES =",
                    r"0x80000000u", r"__builtin_amdgcn_global_load_lds\(", r"__builtin_amdgcn_raw_buffer_load_b32\(", r"s_waitcnt vmcnt\(0\)",
                    r"ecm_allow_lds\(", r"hipLaunchKernelGGL\(kern,"):
        assert len(re.findall(pattern, stage)) == 1, pattern
        for u in users:
            assert not re.search(pattern, u), pattern
    for u in users:                                                     # kernel and launcher read the one LDS_BYTES
        assert len(re.findall(r"Cfg::Stage::LDS_BYTES", u)) == 1 and len(re.findall(r"stage_run<G, (true|false), (true|false)>\(smem, tid,", u)) == 1
    common = _read("csrc", "common.h")
    assert len(re.findall(r"constexpr int mfma32_row\(", common)) == 1 and "mfma32_row" not in _read("csrc", "bf16.h")
    srcs = [_read("csrc", f) for f in sorted(os.listdir(os.path.join(PKG, "csrc"))) if f.endswith((".hip", ".h"))]
    assert sum(len(re.findall(r"8 \* \(i >> 2\)", s)) for s in srcs) == 1       # the map is spelled out in mfma32_row alone
    return _constexpr(stage, "TW", "fp32_conv_stage.h")


def test_stage_constants_exist_once():
    assert stage_constants_exist_once() == T.TW


def _body(src, head):
    """The text of the function whose definition starts with `head`, up to the first line that is a lone closing brace."""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_direct_forward_dispatch_is_that_of_the_source():
    src = _read("csrc", "conv3d.hip")
    assert stage_constants_exist_once() == T.TW
    body = _body(src, 'extern "C" int ecm_conv3d_k3_fwd(')
    assert "if (Ci % 4 != 0 || Co < 1 || Co > 64 || (stride != 1 && stride != 2)) return ECM_EUNSUP;" in body
    assert "const bool two = Co > 32;" in body
    assert "(long long)B * ((Do + 1) / 2) * ((Ho + 7) / 8) * ((Wo + TW - 1) / TW);" in body
    assert _ints(body, r"const bool small = big_blocks < (\d+);", "the small threshold") == (T.SMALL_BLOCKS,)
    got = [tuple(map(int, m)) for m in re.findall(r"launch_conv<(\d+), (\d+), (\d+), (\d+), (\d+)>\(", body)]
    # the source's order: stride 1 then 2, one then two channel tiles, `small ? a : b`
    want = [T.FWD_INST[(s, two, small)] for s in (1, 2) for two in (False, True) for small in (True, False)]
    assert got == want
    assert "if (stride == 1) {" in body and body.count("small ?") == 4 and body.count("if (!two) return small") == 2
    launch = _body(src, "int launch_conv(")
    assert "tiles_d = (Do + TD - 1) / TD, tiles_h = (Ho + TH - 1) / TH, tiles_w = (Wo + TW - 1) / TW;" in launch
    xcd = _body(_read("csrc", "common.h"), "__device__ __forceinline__ int ecm_xcd_tile(")
    assert "x * q + (x < r ? x : r) + (id >> 3)" in xcd


def test_weight_gradient_dispatch_is_that_of_the_source():
    src = _read("csrc", "conv3d_wgrad.hip")
    assert (_constexpr(src, "CT", "conv3d_wgrad.hip"), _constexpr(src, "TWV", "conv3d_wgrad.hip")) == (T.CT, T.TWV)
    # one selector per family names the instantiations; the query and the entry point both go through it to plan<Cfg>
    sel = _body(src, "int wg3_select(")
    assert "wg_select<WgCfg<%d, %d, %d, %d>, WgCfg<%d, %d, %d, %d>>(" % (T.WGRAD_INST["s1"] + T.WGRAD_INST["s2"]) in sel
    assert "decltype(c)::S == stride" in sel and len(re.findall(r"WgCfg<", sel)) == 2
    assert "wg_select<WgCfg<1, %d, %d, %d>, WgCfg<" % T.WGRAD_INST["wino"] in _body(src, "int wgw_select(")
    assert "decltype(c)::KD == kd" in _body(src, "int wgw_select(")
    for fn in ('extern "C" long long ecm_conv3d_wgrad_scratch_bytes(', 'extern "C" int ecm_conv3d_k3_wgrad('):
        assert "wg3_select(stride, [&](auto c) {" in _body(src, fn)
        assert "(B, Ci, Co, wg_out(D, stride), wg_out(H, stride), wg_out(W, stride));" in _body(src, fn)
    assert "inline int wg_out(int n, int stride) { return (n - 1) / stride + 1; }" in src
    assert "return launch_wgrad<Cfg>(" in _body(src, 'extern "C" int ecm_conv3d_k3_wgrad(')
    assert "conv3d_wgrad_mfma<Cfg::S, Cfg::TD, Cfg::TH, Cfg::KD, Cfg::KH, Cfg::KW, Cfg::DIL>" in _body(src, "int launch_wgrad(")
    assert "conv3d_wgrad_mfma<1, Cfg::TD, Cfg::TH, Cfg::KD, 3, 3, 1, true>" in _body(src, "int launch_wgrad_wino(")
    for fn in ('extern "C" long long ecm_conv_wino_wgrad_scratch_bytes(', 'extern "C" int ecm_conv_wino_wgrad('):
        assert "wgw_select(kd, [&](auto c) {" in _body(src, fn) and "true>(B, Ci, Co, D, H, W);" in _body(src, fn)
    workers = _body(src, "WgPlan plan(")
    assert "p.ci_tiles = (Ci + CT - 1) / CT; p.co_tiles = (Co + CT - 1) / CT;" in workers
    assert _ints(workers, r"long long workers = (\d+) \* Cfg::OCC / \(p\.ci_tiles \* p\.co_tiles\);", "workers") == (T.WGRAD_WORKERS,)
    assert "if (workers < 1) workers = 1;" in workers and "if (workers > p.ntiles) workers = p.ntiles;" in workers
    # the occupancy is one number: WgCfg::OCC, read by the kernel's launch bounds and by plan()
    assert src.count("static constexpr int OCC = KD == 3 ? 1 : 2;") == 1 and src.count("KD == 3 ? 1 : 2") == 1 and T.WGRAD_OCC3D == 1
    assert "__launch_bounds__(256, (WgCfg<STRIDE, TD, TH, KD, KH, KW, DIL>::OCC)) void conv3d_wgrad_mfma(" in src
    # tile counts: TWV columns; the Winograd form tiles the (stride-1) volume itself (its plan is given D, H, W)
    assert ("p.tiles_d = (Do + Cfg::TD - 1) / Cfg::TD; p.tiles_h = (Ho + Cfg::TH - 1) / Cfg::TH; p.tiles_w = (Wo + TWV - 1) / TWV;"
            in workers)
    for gone in ("ntiles_for", "ntiles_wino", "ntiles2d_ex", "WG2(", "wgrad_workers", "wgrad_reduce"):
        assert gone not in src, gone
    # the persistent schedule worker_runs restates
    for line in ("if ((gridDim.x & 7u) == 0u) {", "const unsigned start = xcd * q + (xcd < rr ? xcd : rr);",
                 "tile0 = start + (blockIdx.x >> 3);", "tile_end = start + q + (xcd < rr ? 1u : 0u);", "tile_step = gridDim.x >> 3;",
                 "for (unsigned tile = tile0; tile < tile_end; tile += tile_step) {"):
        assert line in src, line
    assert T.worker_runs(64, 90)[:8] == [2] * 8 and sorted(set(T.worker_runs(64, 90))) == [1, 2] and sum(T.worker_runs(64, 90)) == 90
    assert T.worker_runs(42, 48) == [2] * 6 + [1] * 36 and T.worker_runs(16, 18).count(2) == 2


def test_winograd_dispatch_is_that_of_the_source():
    src = _read("csrc", "conv_wino.hip")
    assert _ints(src, r"^constexpr int WINO_CIC3 = (\d+), WINO_CIC2 = \d+;", "WINO_CIC3") == (T.WINO_CIC3,)
    assert "if (kd == 3) return launch_wino<%d, %d, %d, WINO_CIC3>(" % T.WINO_INST[:3] in src
    launch = _body(src, "int launch_wino(")
    assert "tiles_wt = (W + 1) / 2, ntile = ((H + 1) / 2) * tiles_wt;" in launch
    assert _ints(launch, r"const int tblocks = \(ntile \+ (\d+) \* TR - 1\) / \((\d+) \* TR\);", "tile block") == (T.WINO_BLOCK,) * 2
    assert "const int groups = (Co + 31) / 32, nchunks = (Ci + CIC - 1) / CIC;" in launch
    assert "if (W < 2) return ECM_EUNSUP;" in src
    ops = _read("ops.py")
    assert "    return WINOGRAD and x.shape[-1] >= 2 and vol * 128 <= 0x80000000\n" in _body(ops + "\n}\n", "def _wino_ok(x):")
    assert "    return w.shape[0] == 1 and stride == 1 and w.shape[1] <= 32 and w.shape[1] % 8 == 0\n" in ops
    assert "    if stride == 1 and _wino_ok(x) and WINOGRAD_WGRAD:\n        return _wino_wgrad(x, gy, Co, Ci, 3, w)" in ops
    assert T.wino_ok((4, 6, 2)) and not T.wino_ok((4, 6, 1)) and not T.wino_ok((4, 6, 8), False) and not T.wino_ok((256, 256, 257))
    assert T.is_c1(1, 32, 1) and T.is_c1(1, 8, 1) and not T.is_c1(1, 12, 1) and not T.is_c1(1, 40, 1) and not T.is_c1(1, 32, 2)


def test_deconv_and_c1_constants_are_those_of_the_sources():
    src = _read("csrc", "deconv3d.hip")
    assert stage_constants_exist_once() == T.TW
    assert _ints(src, r"static constexpr int TD = (\d+), TH = (\d+), NTAPS = 9 \* KD;", "DeconvCfg") == (T.DECONV_TD, T.DECONV_TH)
    body = _body(src, 'extern "C" int ecm_deconv3d_k3s2_fwd(')
    assert "if (Co > 32) return launch_deconv<%d, %d>(" % T.DECONV_INST[True] in body
    assert "    return launch_deconv<%d, %d>(" % T.DECONV_INST[False] in body
    assert "if (Ci % 4 != 0 || Co < 1 || Co > 64) return ECM_EUNSUP;" in body
    assert "tiles_d = (D + Cfg::TD - 1) / Cfg::TD, tiles_h = (H + Cfg::TH - 1) / Cfg::TH, tiles_w = (W + TW - 1) / TW;" in src
    c1 = _read("csrc", "conv3d_c1.hip")
    got = {n: _constexpr(c1, n, "conv3d_c1.hip") for n in ("VT_W", "VT_H", "VT_D", "DTH", "DTW", "GTD", "GTH", "GTW")}
    assert got == {n: getattr(T, n) for n in got}
    plan = _body(c1, "inline C1WgPlan c1_wgrad_plan(")                  # read by the scratch query and by the launcher
    assert _ints(plan, r"p\.P = \(int\)\(p\.ntiles < (\d+) \? p\.ntiles : (\d+)\);", "workers") == (T.C1_WORKERS,) * 2
    assert "p.tiles_d = (D + GTD - 1) / GTD; p.tiles_h = (H + GTH - 1) / GTH; p.tiles_w = (W + GTW - 1) / GTW;" in plan
    assert "p.ntiles = (long long)B * p.tiles_d * p.tiles_h * p.tiles_w;" in plan
    assert c1.count("c1_wgrad_plan(B, Ci, D, H, W);") == 2 and "c1_workers" not in c1 and "c1_tiles" not in c1
    assert "for (unsigned tile = blockIdx.x; tile < (unsigned)ntiles; tile += gridDim.x) {" in c1
    assert "if (valu && Ci % 2 == 0) return launch_c1_fwd_v<false>(" in c1


def test_restated_dispatch_on_known_shapes():
    """The figures the sources and the issue quote: the step's 48 x 144 x 240 volume takes the large tiles, the hourglass's
    1/16 level the small one; 64 -> 64 weight gradients run 64 workers; 612 tiles of the 32 -> 1 layer meet 512 workers."""
    assert T.direct_fwd(4, 32, 32, (48, 144, 240), 1)["inst"] == (1, 1, 4, 8, 4)
    assert T.direct_fwd(4, 32, 64, (48, 144, 240), 2)["inst"] == (2, 2, 2, 8, 2)
    assert T.direct_fwd(4, 64, 64, (12, 36, 60), 1)["inst"] == (2, 1, 1, 4, 4)
    g = T.direct_fwd(4, 32, 32, (49, 9, 33), 1)
    assert not g["small"] and g["nblk"] == 4 * 13 * 2 * 2 and g["ragged"] == (True, True, True)
    assert T.direct_fwd(3, 32, 32, (49, 9, 33), 1)["small"]                     # 300 blocks: below the threshold
    g = T.wgrad_geom("s1", 2, 64, 64, (10, 17, 33))
    assert (g["P"], g["ntiles"]) == (64, 90)
    g = T.wgrad_geom("wino", 2, 40, 72, (5, 10, 50))
    assert (g["ytiles"], g["P"], g["ntiles"]) == (6, 42, 48)
    assert T.wgrad_geom("s1", 1, 128, 128, (5, 9, 33))["P"] == 16
    g = T.c1_geom(6, 8, (33, 17, 33))
    assert g["wgrad_tiles"] == 612 and g["wgrad_P"] == 512 and g["wgrad_runs"].count(2) == 100
    g = T.wino_geom(1, 2, 8, (3, 5, 6))
    assert (g["tiles_wt"], g["ntile"], g["tblocks"], g["nchunks"]) == (3, 9, 1, 1)


def test_every_path_class_has_a_case():
    assert T.missing_classes() == []
    reached = {(fam, g["inst"]) for c in T.CASES.values() for _, fam, g in T.launches(c) if "inst" in g}
    assert {i for f, i in reached if f == "direct"} == set(T.FWD_INST.values())
    assert {i for f, i in reached if f == "wgrad"} == set(T.WGRAD_INST.values())
    assert {i for f, i in reached if f == "deconv"} == set(T.DECONV_INST.values())
    names = {c for c in T.CASES.values()}
    assert len(names) == len(T.CASES), "two cases share one specification"


def test_the_check_can_fail(monkeypatch):
    """A retuned threshold moves the large-tile cases onto the small tile, and missing_classes() says so."""
    monkeypatch.setattr(T, "SMALL_BLOCKS", 512)
    missing = T.missing_classes()
    assert any("(1, 1, 4, 8, 4)" in m for m in missing) and any("(2, 2, 2, 8, 2)" in m for m in missing)


def test_winograd_restatement_is_the_convolution_in_fp64():
    """The third candidate of the unit evaluates the same operation: the check of the GPU module, run here too."""
    for shape in T.RESTATEMENT_SHAPES:
        T.test_winograd_restatement_is_the_convolution(shape)
    x, w = T.seeded("c3.rs.x", 1, 2, 2, 4, 5), T.seeded("c3.rs.w", 3, 2, 3, 3, 3)
    assert T.wino_fwd(x, w).dtype == torch.float32 and T.wino_wgrad(x, T.wino_fwd(x, w)).shape == w.shape


def test_chain_restatement_is_the_convolution_in_fp64():
    """The summation-order candidate of the direct kernel's unit evaluates the same operation: the check of the GPU module, here too."""
    for stride in (1, 2):
        T.test_chain_restatement_is_the_convolution(stride)
