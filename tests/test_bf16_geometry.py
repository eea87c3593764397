"""The case table of tests/test_hip_bf16_fp64.py, checked without a GPU: its restatement of the host-side dispatch of the bf16
inference convolutions uses the constants, thresholds and template arguments of csrc/bf16_conv2d.h, bf16_encoder.hip,
bf16_decoder.hip, bf16_conv3d.h, bf16_infer.hip, conv3d_c1.hip and ops.py as they stand in the sources (a retune of KC, TW, NT or
a tile shape must not silently move the cases off the paths they were chosen for), every class has a case, every case is inside
the kernels' contracts, `rne_bf16` is the rounding it claims to be, and the operands meet three conditions:
  * for every bf16-output case at most UNDECIDED_CAP = 2 % of the outputs are undecided, i.e. rne_bf16(y64 - b0) != rne_bf16(y64 + b0)
    with b0 = K * e32 + FLOOR * max|y64| built from the CPU's fp32 evaluation alone (the GPU test asserts the same cap with its full
    bound).  t_s2_one (one undecided output of 64) and t_s1_ragged came within a quarter of the cap under their plain names and
    carry a salt for that reason;
  * for every conv2d_c1_relu_bf16 case between 25 % and 75 % of the reference outputs are positive (the bias is the negated
    median of the sums), so both sides of the ReLU are exercised;
  * one deconv2d_k3s2_bias_bf16 case has a bias of magnitude 50 against sums of order 1, and a bias added AFTER the rounding
    fails that case's interval."""
import re

import pytest
import torch

import test_hip_bf16_fp64 as T
from test_conv3d_geometry import _body, _constexpr, _ints, _read

BF16_OUT = sorted(n for n, c in T.CASES.items() if T.bf16_out(c))


# ---- the sources ---------------------------------------------------------------------------------------------------------------
def test_stage2d_pipeline_is_that_of_the_source():
    src = _read("csrc", "bf16_conv2d.h")
    assert _constexpr(src, "KC", "bf16_conv2d.h") == T.KC
    run = _body(src, "__device__ __forceinline__ void stage2d_run(")
    assert "const int nchunks = Ci / KC;" in run
    # the four phases of the double-buffered loop the case table enumerates by chunk count
    for line in ("    fetch(0);\n    store(0);\n    if (nchunks > 1) fetch(1);\n    __syncthreads();\n", "for (int ch = 0; ch < nchunks; ++ch) {",
                 "const int buf = ch & 1;", "if (ch + 1 < nchunks) {", "store(buf ^ 1);", "if (ch + 2 < nchunks) fetch(ch + 2);"):
        assert line in run, line
    assert "void (*const kern)(P...) = vec ? kvec : kany;" in _body(src, "int stage2d_launch(")
    assert "if (VEC) m = (unsigned)gx < (unsigned)W ? 0xffu : 0u;" in src


def test_encoder_dispatch_is_that_of_the_source():
    src = _read("csrc", "bf16_encoder.hip")
    assert _constexpr(src, "TW", "bf16_encoder.hip") == T.TW
    geo = _body(src + "\n}\n", "struct Geo2 {")
    for line in ("static constexpr int PAD = DL * (KS - 1) / 2;", "static constexpr int TH = 4 * NT;",
                 "static constexpr int HR = S * (TH - 1) + DL * (KS - 1) + 1;", "static constexpr int XOFF = PAD ? 8 - PAD : 0;",
                 "static constexpr int IWP = (XOFF + S * (TW - 1) + DL * (KS - 1) + 1 + 7) / 8 * 8;"):
        assert line in geo, line
    disp = _body(src, "int dispatch(")
    assert "const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;" in disp
    for (k, s, d), nt in T.ENC_NT.items():
        assert ("if (k == %d && stride == %d && dil == %d) return launch_co<%d, %d, %d, %d>(x, wp, y, B, Ci, Co, H, W, Ho, Wo, stream);"
                % (k, s, d, k, s, d, nt)) in disp
    assert disp.count("launch_co<") == len(T.ENC_NT) == 6 and "return ECM_EUNSUP;" in disp
    co = _body(src, "int launch_co(")
    assert ("    if constexpr (KS == 1 && S == 1)\n        if (Co % 128 == 0) return launch_enc<KS, S, DL, NT, 4, OutT>(") in co
    assert "    if (Co % 64 == 0) return launch_enc<KS, S, DL, NT, 2, OutT>(" in co
    assert "    return launch_enc<KS, S, DL, NT, 1, OutT>(" in co and co.count("launch_enc<") == 3
    enc = _body(src, "int launch_enc(")
    assert "constexpr int TH = 4 * NT;" in enc and "const int th = (Ho + TH - 1) / TH, tw = (Wo + TW - 1) / TW;" in enc
    assert "conv2d_bf16<KS, S, DL, NT, COT, true, OutT>, conv2d_bf16<KS, S, DL, NT, COT, false, OutT>, W % 8 == 0," in enc
    assert "dim3((unsigned)nb, (unsigned)(Co / (COT * 32)))" in enc
    fwd = _body(src, 'extern "C" int ecm_conv2d_bf16_fwd(')
    assert "if (Ci % KC != 0 || Co % 32 != 0) return ECM_EUNSUP;" in fwd
    assert "if (out_f32) return dispatch<float>(x, wpacked, static_cast<float*>(y), B, Ci, Co, H, W, k, stride, dil, stream);" in fwd
    assert "return dispatch<u16>(x, wpacked, static_cast<u16*>(y), B, Ci, Co, H, W, k, stride, dil, stream);" in fwd
    # the kernel's use of the grid and its epilogue guards
    for line in ("const int cb = blockIdx.y;", "const int oh0 = th * TH, ow0 = tw * TW;", "if (ow >= Wo) return;", "if (oh >= Ho) continue;",
                 "OutT* yb = y + ((size_t)b * Co + cb * COP) * HWo;"):
        assert line in src, line
    ops = _read("ops.py")
    assert "int(out_dtype == torch.float32), _stream())" in ops
    for k, s, d in T.ENC_NT:                                                # the window of every kind is whole 8-column segments
        g = T.geo2(k, s, d, T.ENC_NT[(k, s, d)])
        assert g["IWP"] % 8 == 0 and g["PAD"] <= 8 and g["IWP"] >= g["XOFF"] + s * (T.TW - 1) + d * (k - 1) + 1
    assert T.geo2(3, 1, 1, 2) == dict(PAD=1, TH=8, HR=10, XOFF=7, IWP=48) and T.geo2(1, 2, 1, 2)["IWP"] == 64


def test_decoder_dispatch_is_that_of_the_source():
    src = _read("csrc", "bf16_decoder.hip")
    got = tuple(_constexpr(src, n, "bf16_decoder.hip") for n in ("DTW", "DTH", "DIWP", "C1R"))
    assert got == (T.DTW, T.DTH, T.DIWP, T.C1R) and T.DIWP == (T.DTW + 1 + 7) // 8 * 8
    a, b = _ints(src, r"^constexpr int C1W = (\d+) \* (\d+);", "C1W")
    assert (a, a * b) == (64, T.C1W)                                        # 64 lanes of 8 columns
    a, b = _ints(src, r"^constexpr int C1MAXW = (\d+) \* (\d+);", "C1MAXW")
    assert a * b == T.C1MAXW
    assert "using DecStage = Stage2d<DHR, DIWP, 9, COT>;" in src
    dec = _body(src, "int launch_dec(")
    assert "const int th = (H + DTH - 1) / DTH, tw = (W + DTW - 1) / DTW;" in dec
    assert "stage2d_launch(deconv2d_bf16<COT, true>, deconv2d_bf16<COT, false>, W % 8 == 0, dim3((unsigned)nb), DecStage<COT>::LDS_BYTES," in dec
    fwd = _body(src, 'extern "C" int ecm_deconv2d_k3s2_bias_bf16_fwd(')
    assert "if (Ci % KC != 0 || (Co != 32 && Co != 64)) return ECM_EUNSUP;" in fwd
    assert "if (Co == 64) return launch_dec<2>(" in fwd and "    return launch_dec<1>(" in fwd
    for line in ("const int i0 = th * DTH, j0 = tw * DTW;", "const int i = i0 + wave, j = j0 + l31;", "if (i >= H || j >= W) return;"):
        assert line in src, line
    c1 = _body(src, 'extern "C" int ecm_conv2d_c1_bf16_fwd(')
    assert "if (Ci % KC != 0 || 9 * Ci > C1MAXW || (long long)H * W >= 0x7fffffffLL) return ECM_EUNSUP;" in c1
    assert "const int th = (H + 4 * C1R - 1) / (4 * C1R), tw = (W + C1W - 1) / C1W;" in c1
    assert "    if (W % 8 == 0)\n        hipLaunchKernelGGL((conv2d_c1_bf16<true>), dim3((unsigned)nb), dim3(256)," in c1
    assert "    else\n        hipLaunchKernelGGL((conv2d_c1_bf16<false>), dim3((unsigned)nb), dim3(256)," in c1 and T.C1_WAVES * 64 == 256
    for line in ("const int r0 = (th * 4 + wave) * C1R;", "const int c0 = tw * C1W + lane * 8;", "if (r0 >= H) return;", "if (gy >= H) break;",
                 "const int ec = lane == 0 ? c0 - 1 : c0 + 8;", "if (c0 < W) {", "if (c0 + c < W) dst[c] = o[c];"):
        assert line in src, line
    ops = _read("ops.py")
    assert "and x.shape[1] % 16 == 0 and x.shape[1] <= 1024," in _body(ops + "\n}\n", "def conv2d_c1_relu_bf16(")


def test_taps_dispatch_is_that_of_the_source():
    src = _read("csrc", "bf16_infer.hip")
    got = _ints(src, r"^constexpr int S1_TD = (\d+), S1_TH = (\d+), S2_TD = (\d+), S2_TH = (\d+), DC_TD = (\d+), DC_TH = (\d+);", "tile shapes")
    assert got == T.TAPS_TILE[0] + T.TAPS_TILE[1] + T.TAPS_TILE[2]
    conv = _body(src, 'extern "C" int ecm_conv3d_k3_bf16_fwd(')
    assert "const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;" in conv
    got = re.findall(r"(return Co == 32 \?|:) launch_conv3d_taps<Bf16Op, (\d), (\d), (S\d)_TD, (S\d)_TH>\(", conv)
    assert got == [("return Co == 32 ?", "1", "0", "S1", "S1"), (":", "2", "0", "S1", "S1"),
                   ("return Co == 32 ?", "1", "1", "S2", "S2"), (":", "2", "1", "S2", "S2")]
    assert "if (stride == 1)\n" in conv and "if (!conv_shape_ok(Ci, Co, D, H, W)) return ECM_EUNSUP;" in conv
    dc = _body(src, 'extern "C" int ecm_deconv3d_k3s2_bf16_fwd(')
    got = re.findall(r"(return Co == 32 \?|:) launch_conv3d_taps<Bf16Op, (\d), 2, DC_TD, DC_TH>\(x, wpacked, y, B, Ci, D, H, W, 2 \* D, 2 \* H, 2 \* W, stream\)", dc)
    assert got == [("return Co == 32 ?", "1"), (":", "2")]
    assert src.count("launch_conv3d_taps<Bf16Op") == 6 and "return taps_channels_ok(Ci, Co) &&" in src
    hdr = _read("csrc", "bf16_conv3d.h")
    assert _constexpr(hdr, "TW", "bf16_conv3d.h") == T.TW
    assert "constexpr bool taps_channels_ok(int Ci, int Co) { return (Ci == 32 || Ci == 64) && (Co == 32 || Co == 64); }" in hdr
    launch = _body(hdr, "int launch_conv3d_taps(")
    assert "const int gd = MODE == 2 ? D : Do, gh = MODE == 2 ? H : Ho, gw = MODE == 2 ? W : Wo;" in launch
    assert "const int td = (gd + TD - 1) / TD, th = (gh + TH - 1) / TH, tw = (gw + TW - 1) / TW;" in launch
    assert "dim3((unsigned)nb, MODE == 2 ? 8 : 1)" in launch
    body = _body(hdr, "__device__ __forceinline__ void conv3d_taps_body(")
    for line in ("for (int c0 = 0; c0 < Ci; c0 += %d) {" % T.TAPS_KC, "if (c0 + 8 < Ci) fetch(c0 + 8);", "const int pos = off < 0 ? G::ZERO : rbase[r] + off;",
                 "if (tid < NTERM) Xs[tid * XT + G::ZERO] = make_uint4(0, 0, 0, 0);",
                 "const bool ok = okw && od < Do && oh < Ho && (MODE != 2 || (md < D && mh < H));"):
        assert line in body, line
    assert "switch (blockIdx.y) {" in hdr and hdr.count("ECM_DC_PHASE(") == 8 + 1
    ops = _read("ops.py")
    assert "and x.shape[1] in (32, 64) and w.shape[0] in (32, 64) and x.numel() > 0," in _body(ops + "\n}\n", "def _conv3d_bf16(")
    assert "and x.shape[1] in (32, 64) and w.shape[1] in (32, 64) and x.numel() > 0," in _body(ops + "\n}\n", "def _deconv3d_bf16(")


def test_tail_dispatch_is_that_of_the_source():
    src = _read("csrc", "conv3d_c1.hip")
    assert _ints(src, r"^constexpr int VT_W = (\d+), VT_H = (\d+), VT_D = (\d+);", "VT_*") == (T.VT_W, T.VT_H, T.VT_D)
    launch = _body(src, "int launch_c1_fwd_v(")
    assert "const int td = (D + VT_D - 1) / VT_D, th = (H + VT_H - 1) / VT_H, tw = (W + VT_W - 1) / VT_W;" in launch
    fwd = _body(src, 'extern "C" int ecm_conv3d_c1_gn_fwd_bf16(')
    assert "if (Ci != 32 || (long long)D * H * W * 2 * 32 >= 0x7fffffffLL) return ECM_EUNSUP;" in fwd
    assert "return launch_c1_fwd_v<true, unsigned short>(x, w, y, B, Ci, D, H, W, mean_rstd, gamma, beta, stream);" in fwd
    ops = _read("ops.py")
    assert '_lib.call("ecm_conv3d_c1_gn_fwd_bf16", _p(x), _p(stats), _p(gamma), _p(beta), _p(w), _p(y), B, Cc, D, H, W, _stream())' in ops
    assert _ints(ops, r"^GN_EPS = 1e-(\d+)$", "GN_EPS") == (5,) and T.GN_EPS == 1e-5


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_every_class_has_a_case():
    assert T.missing_classes() == []
    inst = T.all_instantiations()
    assert len([i for i in inst if i[0] == "enc"]) == 52 and len(inst) == 52 + 4 + 2 + 6 + 1
    reached = {(g["fam"], g["inst"]) for g in map(T.geom, T.CASES.values())}
    assert reached == set(inst)
    assert len(set(T.CASES.values())) == len(T.CASES), "two cases share one specification"
    assert len(T.ENC) == 52 and set(T.SALT) <= set(T.CASES)


def test_every_case_is_inside_the_contracts():
    """What ops would refuse, or the entry points answer with ECM_EUNSUP, is no case; no production-sized shape is one."""
    import ecm_amd
    ops = ecm_amd.ops
    for name, c in T.CASES.items():
        vol = 1
        for n in c.dims:
            vol *= n
        assert c.B * c.Ci * vol <= 1 << 20 and max(c.dims) <= 520, name
        if c.op == "enc":
            assert ops.conv2d_bf16_supported(c.Ci, c.Co, c.k, c.stride, c.dil) and T.conv2d_bf16_supported(c.Ci, c.Co, c.k, c.stride, c.dil), name
        elif c.op == "dec":
            assert ops.deconv2d_bf16_supported(c.Ci, c.Co) and c.Co in (32, 64) and c.Ci % T.KC == 0, name
        elif c.op == "c1":
            assert c.Ci % 16 == 0 and c.Ci <= 1024 and 9 * c.Ci <= T.C1MAXW and c.Co == 1, name
        elif c.op in ("c3", "dc3"):
            assert c.Ci in (32, 64) and c.Co in (32, 64) and c.stride in (1, 2) and (c.op == "c3" or c.stride == 1), name
        else:
            assert c.op == "tail" and c.Ci == 32 and c.Co == 1, name
        T.geom(c)                                                           # asserts the entry point's own gate
    for args in ((16, 32, 3, 1, 1), (24, 32, 3, 1, 1), (16, 48, 1, 1, 1), (16, 32, 3, 2, 2), (16, 32, 1, 1, 2), (48, 96, 3, 1, 4), (16, 32, 5, 1, 1)):
        assert ops.conv2d_bf16_supported(*args) == T.conv2d_bf16_supported(*args), args


def test_restated_dispatch_on_known_shapes():
    """The shapes the sources and the existing tests quote: the stride-1 1x1 at Co = 128 is the only COT 4; 8 x 64 -> 128 at
    144 x 240 is 8 * 18 * 8 workgroups; the decoder's first level; W = 520 gives conv2d_c1_bf16 two column blocks."""
    g = T.enc_geom(8, 64, 128, 144, 240, 1, 1, 1, False)
    assert g["inst"] == (1, 1, 1, 2, 4, True, "bf16") and g["grid"] == (8 * 18 * 8, 1) and g["chunks"] == 4
    assert T.enc_geom(1, 16, 128, 8, 8, 3, 1, 1, True)["inst"][4] == 2 and T.enc_geom(1, 16, 128, 8, 8, 1, 2, 1, True)["inst"][4] == 2
    assert T.enc_geom(1, 16, 96, 5, 9, 3, 1, 1, False)["grid"] == (1, 3)
    assert T.dec_geom(12, 96, 64, 144, 240)["grid"] == (12 * 36 * 8, 1) and T.dec_geom(1, 48, 32, 4, 7)["inst"] == (1, False)
    g = T.c1_geom(1, 16, 5, 520)
    assert g["tiles"] == (1, 2) and g["idle_wave"] and g["vec"]
    assert not T.c1_geom(1, 16, 16, 512)["idle_wave"] and T.c1_geom(1, 16, 17, 9)["idle_wave"]
    g = T.taps_geom(1, 64, 64, 9, 9, 40, 1)
    assert g["out"] == (5, 5, 20) and g["tiles"] == (3, 2, 1) and g["chunks"] == 8 and g["grid"] == (6, 1)
    assert T.taps_geom(1, 32, 32, 3, 3, 5, 2)["grid"] == (1, 8)
    assert T.tail_geom(1, 9, 17, 33)["tiles"] == (2, 2, 2)


def test_the_check_can_fail(monkeypatch):
    """A retune moves cases off their classes, and missing_classes() says so."""
    monkeypatch.setattr(T, "TAPS_KC", 16)
    assert any("MODE 0: 8 chunks" in m for m in T.missing_classes())
    monkeypatch.undo()
    monkeypatch.setattr(T, "DTH", 8)
    assert "dec: an exact tile" in T.missing_classes()
    monkeypatch.undo()
    monkeypatch.setattr(T, "C1W", 1024)
    assert any("W crosses 512" in m for m in T.missing_classes())
    monkeypatch.undo()
    assert T.missing_classes() == []


# ---- the rounding and the operands ------------------------------------------------------------------------------------------------
def test_rne_bf16_is_round_to_nearest_even_on_the_fp64_bits():
    v32 = T.seeded("bf.rne", 1 << 16) * torch.logspace(-30, 30, 1 << 16)
    assert torch.equal(T.rne_bf16(v32.double()), v32.bfloat16().double())                    # one rounding either way: they agree
    one, ulp = 1.0, 2.0 ** -7
    v = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -40, -(one + ulp / 2 + 2.0 ** -40), one + ulp / 2 - 2.0 ** -40,
                      0.0, 2.0 - 2.0 ** -9, 2.0 ** -126 * (1 + ulp / 2), 2.0 ** -133 * 2.5, 2.0 ** -133 * 3.5, 2.0 ** -134],
                     dtype=torch.float64)
    want = torch.tensor([one, one + 2 * ulp, one + ulp, -(one + ulp), one, 0.0, 2.0, 2.0 ** -126, 2.0 ** -133 * 2, 2.0 ** -133 * 4, 0.0],
                        dtype=torch.float64)
    assert torch.equal(T.rne_bf16(v), want)
    assert float(v[2].float().bfloat16()) == one                                             # the detour through fp32 rounds twice
    got = T.rne_bf16(v)
    assert torch.equal(got.float().bfloat16().double(), got)                                 # the results are bf16 values
    lo, hi = T.interval(torch.tensor([1.0, 1.0 + ulp / 2], dtype=torch.float64), 1e-6)
    assert lo.tolist() == [1.0, 1.0] and hi.tolist() == [1.0, 1.0 + ulp]


@pytest.mark.parametrize("name", BF16_OUT)
def test_undecided_share(name):
    share = T.cpu_conditions(name)["undecided"]
    assert share <= T.UNDECIDED_CAP, (name, share)


@pytest.mark.parametrize("name", sorted(n for n, c in T.CASES.items() if c.op == "c1"))
def test_relu_sees_both_sides(name):
    positive = T.cpu_conditions(name)["positive"]
    assert 0.25 <= positive <= 0.75, (name, positive)


def test_large_bias_case_is_sharp():
    """d_bias50: |b| = 50 against sums of order 1; rounding the sum and THEN adding the bias (a second rounding) leaves the interval,
    and so does an accumulator that is truncated to bf16 instead of rounded."""
    o, y64, y32 = T.reference("d_bias50")
    assert bool((o["b"].abs() == 50.0).all()) and 1.0 <= float((y64 - o["b"].double().view(1, -1, 1, 1)).abs().max()) <= 8.0
    lo, hi = T.interval(y64, T.K * float((y32.double() - y64).abs().max()) + T.FLOOR * float(y64.abs().max()))
    inside = lambda y: bool(((lo <= y.double()) & (y.double() <= hi)).all())                   # noqa: E731
    assert inside(y32.bfloat16())
    twice = ((y32 - o["b"].view(1, -1, 1, 1)).bfloat16().float() + o["b"].view(1, -1, 1, 1)).bfloat16()
    assert not inside(twice)
    truncated = (y32.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert not inside(truncated)


@pytest.mark.parametrize("name", ["e_k3s1d1_co32_vec_bf16_exact", "d_ragged", "t_s1_one", "e_one"])
def test_the_interval_rejects_a_truncating_kernel(name):
    """Even the smallest bf16-output cases tell round-to-nearest-even from truncation (what the 1-ulp bar of the older tests
    cannot): the fp32 evaluation rounded once lies inside the interval, the same values truncated do not."""
    _, y64, y32 = T.reference(name)
    lo, hi = T.interval(y64, T.K * float((y32.double() - y64).abs().max()) + T.FLOOR * float(y64.abs().max()))
    rounded, truncated = y32.bfloat16().double(), (y32.view(torch.int32) & -65536).view(torch.float32).double()
    assert bool(((lo <= rounded) & (rounded <= hi)).all())
    assert not bool(((lo <= truncated) & (truncated <= hi)).all())
