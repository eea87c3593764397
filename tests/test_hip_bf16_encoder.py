"""The opt-in bf16 encoder (ops.encoder_dtype) on the MI355X.

Kernel parity: the bf16 convolution and the bf16-in / fp32-out GroupNorm against F.conv2d / F.group_norm in fp32 on the same
bf16-rounded operands -- bf16 outputs within 1 bf16 ulp of that yardstick rounded to bf16 (or 1e-5 of max |y| where a value is
tiny), fp32 outputs within fp32 accumulation-order tolerance.  Whole models: the HIP bf16 disparities against a reference R (the
fp64 fixtures where they exist, else the fp32 HIP output) within 2x the mean and 4x the max distance of an EMULATION: the
library's fp32 kernels fed and followed by bf16 rounding at exactly the bf16 encoder's rounding points (the emulated maps ARE
bf16 tensors between layers; every convolution and GroupNorm computes in fp32 on their values).

The per-path numerical check of these kernels (every instantiation against fp64, once-rounded outputs, repeats on poisoned
memory) is tests/test_hip_bf16_fp64.py with tests/test_bf16_geometry.py; the bars below are kept as they were."""
import contextlib
import time

import pytest
import torch
import torch.nn.functional as F

from oracle.weights import seeded
from test_hip_bf16_infer import ARCHS, _emulated, _fp32_accepts, _model, _within_ulp, _z
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def _R(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


def _within_f32(got, want, label):
    err = (got - want).abs()
    tol = 2e-5 * float(want.abs().max()) + 1e-4 * want.abs()
    assert bool((err <= tol).all()), f"{label}: worst excess {float((err - tol).max()):.3e}"


# ------------------------------------------------------------------------------------------------ kernel parity
# (B, Ci, Co, (H, W), k, stride, dilation): every layer kind of the five encoder variants at 8 images of 576x960 (maps 576x960,
# 288x480, 144x240, SPP branches down to 2x3) and of 384x1248 (96x312), then awkward sizes (w = 78, 33, 1, odd h), then a single
# 16-channel chunk (the chunk loop without a prefetch) with 2-byte and with 16-byte row loads, 32 and 64 channels per workgroup
_CONV = [(8, 32, 32, (576, 960), 3, 1, 1), (8, 32, 32, (288, 480), 3, 1, 1), (8, 64, 64, (144, 240), 3, 1, 1),
         (8, 64, 128, (144, 240), 3, 1, 1), (8, 128, 128, (144, 240), 3, 1, 1), (8, 320, 128, (144, 240), 3, 1, 1),
         (8, 384, 128, (144, 240), 3, 1, 1),
         (8, 64, 128, (144, 240), 3, 1, 2), (8, 128, 128, (144, 240), 3, 1, 2), (8, 128, 128, (144, 240), 3, 1, 4),
         (8, 32, 32, (576, 960), 3, 2, 1), (8, 32, 64, (288, 480), 3, 2, 1), (8, 64, 128, (288, 480), 3, 2, 1),
         (8, 64, 128, (144, 240), 1, 1, 1), (8, 128, 32, (144, 240), 1, 1, 1), (8, 128, 32, (18, 30), 1, 1, 1),
         (8, 128, 32, (2, 3), 1, 1, 1),
         (8, 32, 32, (576, 960), 1, 2, 1), (8, 32, 64, (288, 480), 1, 2, 1), (8, 64, 128, (288, 480), 1, 2, 1),
         (8, 128, 128, (96, 312), 3, 1, 2), (8, 64, 64, (96, 312), 3, 1, 1), (8, 32, 32, (384, 1248), 3, 2, 1),
         (1, 32, 32, (7, 78), 3, 1, 1), (1, 64, 128, (24, 78), 3, 1, 4), (2, 128, 128, (5, 33), 3, 1, 2),
         (1, 32, 64, (9, 33), 3, 2, 1), (2, 64, 128, (3, 1), 3, 2, 1), (1, 128, 32, (1, 1), 1, 1, 1), (1, 64, 128, (5, 33), 1, 2, 1),
         (1, 384, 128, (13, 312), 3, 1, 1), (1, 32, 32, (1, 1), 3, 1, 1), (2, 128, 32, (11, 78), 1, 1, 1),
         (1, 16, 32, (5, 33), 3, 1, 1), (1, 16, 32, (4, 40), 1, 1, 1), (1, 16, 64, (5, 33), 3, 2, 1)]


@pytest.mark.parametrize("B,Ci,Co,hw,k,stride,dil", _CONV)
def test_conv2d_bf16_parity(ecm, B, Ci, Co, hw, k, stride, dil):
    x = _R(B, Ci, *hw, seed=1, dtype=BF)
    w = _R(Co, Ci, k, k, seed=2, scale=(2.0 / (k * k * Co)) ** 0.5)
    with torch.no_grad(), torch.backends.cudnn.flags(allow_tf32=False):
        y = ecm.ops.conv2d_bf16(x, w, stride, dil)
        want = F.conv2d(x.float(), w.bfloat16().float(), stride=stride, padding=dil * (k - 1) // 2, dilation=dil)
    assert y.dtype == BF and y.shape == want.shape and y.is_contiguous()
    _within_ulp(y, want, f"conv2d {B}x{Ci}->{Co} {hw} k{k} s{stride} d{dil}")


@pytest.mark.parametrize("B,Ci,Co,hw,k", [(8, 32, 32, (576, 960), 3), (8, 128, 32, (144, 240), 1), (8, 32, 32, (384, 1248), 3),
                                          (1, 32, 32, (7, 78), 3), (2, 128, 32, (5, 33), 1), (1, 32, 32, (1, 1), 3),
                                          (1, 16, 32, (5, 33), 3)])
def test_conv2d_bf16_fp32_out_parity(ecm, B, Ci, Co, hw, k):
    x = _R(B, Ci, *hw, seed=3, dtype=BF)
    w = _R(Co, Ci, k, k, seed=4, scale=(2.0 / (k * k * Co)) ** 0.5)
    with torch.no_grad(), torch.backends.cudnn.flags(allow_tf32=False):
        y = ecm.ops.conv2d_bf16(x, w, 1, 1, out_dtype=torch.float32)
        want = F.conv2d(x.float(), w.bfloat16().float(), padding=(k - 1) // 2)
    assert y.dtype == torch.float32 and y.shape == want.shape
    _within_f32(y, want, f"conv2d fp32-out {B}x{Ci}->{Co} {hw} k{k}")


_GN = [(8, 32, (576, 960)), (8, 32, (288, 480)), (8, 128, (144, 240)), (1, 32, (7, 78)), (2, 64, (3, 5)), (2, 64, (1, 1))]


@pytest.mark.parametrize("B,Cc,hw", _GN)
@pytest.mark.parametrize("mode", ["relu", "skip", "skip_relu_dual", "relu_dual"])
def test_group_norm_bf16_f32_parity(ecm, B, Cc, hw, mode):
    x = (_R(B, Cc, *hw, seed=5, scale=3.0) + 2.0).to(BF)
    skip = _R(B, Cc, *hw, seed=6, dtype=BF) if "skip" in mode else None
    relu, dual = "relu" in mode, "dual" in mode
    g, b = _R(Cc, seed=7, scale=0.5) + 1.0, _R(Cc, seed=8, scale=0.5)
    with torch.no_grad():
        out = ecm.ops.group_norm_act_bf16_f32(x, g, b, skip, relu, dual=dual)
        want = F.group_norm(x.float(), 32, g, b, eps=1e-5)
        if skip is not None:
            want = want + skip.float()
        if relu:
            want = want.clamp_min(0)
    y32, y16 = out if dual else (out, None)
    assert y32.dtype == torch.float32 and y32.shape == want.shape
    _within_f32(y32, want, f"group_norm fp32-out {mode} {B}x{Cc} {hw}")
    if dual:
        assert y16.dtype == BF and torch.equal(y16, y32.to(BF))               # the same values, rounded once
        _within_ulp(y16, want, f"group_norm dual {mode} {B}x{Cc} {hw}")


def test_conv2d_bf16_keeps_nan(ecm):
    x = _R(1, 32, 4, 40, seed=9, dtype=BF)
    x[0, 0, 1, 5] = float("nan")
    with torch.no_grad():
        y = ecm.ops.conv2d_bf16(x, _R(32, 32, 3, 3, seed=10, scale=0.1))
    assert bool(torch.isnan(y[0, :, 0:3, 4:7]).all())
    assert bool(torch.isfinite(y[0, :, 3:, :]).all())


def test_bf16_conv_outside_contract_raises(ecm):
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="Ci % 16"):
            ecm.ops.conv2d_bf16(_R(1, 24, 4, 8, dtype=BF), _R(32, 24, 3, 3))
        with pytest.raises(RuntimeError, match="Ci % 16"):
            ecm.ops.conv2d_bf16(_R(1, 32, 4, 8, dtype=BF), _R(32, 32, 3, 3), 2, 2)


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B,Ci,Co,hw,k,stride,dil", [(1, 32, 32, (5, 78), 3, 1, 1), (2, 64, 128, (3, 33), 3, 1, 4),
                                                     (1, 32, 64, (7, 33), 3, 2, 1), (1, 128, 32, (2, 3), 1, 1, 1),
                                                     (2, 64, 128, (5, 40), 1, 2, 1), (1, 128, 128, (9, 40), 3, 1, 2),
                                                     (1, 16, 32, (5, 33), 3, 1, 1)])
@pytest.mark.parametrize("out", [BF, torch.float32])
def test_guard_bands_conv2d_bf16(ecm, B, Ci, Co, hw, k, stride, dil, out):
    x, w = _R(B, Ci, *hw, seed=1, dtype=BF), _R(Co, Ci, k, k, seed=2, scale=0.1)
    with torch.no_grad(), guarded(ecm) as g:
        ecm.ops.conv2d_bf16(x, w, stride, dil, out_dtype=out)
        g.check(f"conv2d bf16 {B}x{Ci}->{Co} {hw} k{k} s{stride} d{dil} {out}")


@pytest.mark.parametrize("hw", [(5, 78), (1, 1), (4, 8)])
def test_guard_bands_group_norm_bf16_f32(ecm, hw):
    g32, b32 = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    with torch.no_grad(), guarded(ecm) as g:
        x = _R(2, 32, *hw, seed=1, dtype=BF)
        ecm.ops.group_norm_act_bf16_f32(x, g32, b32, x, True, dual=True)
        ecm.ops.group_norm_act_bf16_f32(x, g32, b32, None, False)
        g.check(f"group_norm bf16 -> fp32 {hw}")


# ------------------------------------------------------------------------------------------------ whole models
@contextlib.contextmanager
def _enc_emulated(ecm):
    """The bf16 encoder's own forward (models.feature_extraction._forward_bf16: same rounding points, bf16 tensors between
    layers) with every new kernel replaced by the library's fp32 kernel on the same bf16 values: a convolution computes in fp32
    on the rounded input and weights and rounds its output once (not at all where it writes fp32); a GroupNorm computes in fp32
    and rounds its output once; the dual GroupNorm returns its fp32 result and that result rounded (what the next layer sees)."""
    ops = ecm.ops
    r = lambda t: t.to(BF).float()
    conv_bf, gn, gn_f32 = ops.conv2d_bf16, ops.group_norm_act, ops.group_norm_act_bf16_f32
    f = lambda t: None if t is None else t.float()

    def conv_e(x, w, stride=1, dil=1, fork=False, out_dtype=BF):
        y = ops.conv2d(x.float(), r(w), stride, dil).to(out_dtype)
        return (y, x) if fork else y

    def gn_e(x, gamma, beta, skip=None, relu=False, head=0, out_dtype=None):
        if x.dtype == BF or out_dtype == BF:
            return gn(x.float(), gamma, beta, f(skip), relu).to(BF)
        return gn(x, gamma, beta, skip, relu, head, out_dtype)

    def gn_f32_e(x, gamma, beta, skip=None, relu=False, dual=False):
        y = gn(x.float(), gamma, beta, f(skip), relu)
        return (y, y.to(BF)) if dual else y

    ops.conv2d_bf16, ops.group_norm_act, ops.group_norm_act_bf16_f32 = conv_e, gn_e, gn_f32_e
    try:
        with ops.encoder_dtype(BF):
            yield
    finally:
        ops.conv2d_bf16, ops.group_norm_act, ops.group_norm_act_bf16_f32 = conv_bf, gn, gn_f32


def _run(ecm, model, left, right, mode):
    """mode: fp32 | enc | enc_emu | both | both_emu"""
    ops = ecm.ops
    with torch.no_grad(), contextlib.ExitStack() as st:
        if mode in ("both", "both_emu"):
            st.enter_context(ops.aggregation_dtype(BF) if mode == "both" else _emulated(ecm))
        if mode in ("enc", "both"):
            st.enter_context(ops.encoder_dtype(BF))
        elif mode.endswith("emu"):
            st.enter_context(_enc_emulated(ecm))        # inside the aggregation emulation: its GroupNorm wrapper sees fp32
        o = model(left, right)
    torch.cuda.synchronize()
    return [t.detach().double().cpu().reshape(-1, *t.shape[-2:]) for t in o]


def _accuracy(ecm, arch, left, right, ref=None, sub=1):
    model = _model(ecm, arch)
    if ref is None:
        ref = _run(ecm, model, left, right, "fp32")
    for mode in ("enc", "both"):
        emu = _run(ecm, model, left, right, mode + "_emu")
        b16 = _run(ecm, model, left, right, mode)
        for i, (r, e, b) in enumerate(zip(ref, emu, b16)):
            e, b = e[..., ::sub, ::sub], b[..., ::sub, ::sub]
            de, db = (e - r).abs(), (b - r).abs()
            row = (float(de.mean()), float(de.max()), float(db.mean()), float(db.max()))
            print(f"{arch} {tuple(left.shape[-2:])} {mode:4s} head {i + 1}: E_mean {row[0]:.3e} E_max {row[1]:.3e} | "
                  f"bf16 mean {row[2]:.3e} max {row[3]:.3e}")
            assert row[2] <= 2 * row[0] and row[3] <= 4 * row[1], (arch, mode, i, row)


@pytest.mark.parametrize("arch", ARCHS)
def test_arch_accuracy_256x512(ecm, arch):
    tag = "g13" if arch == "cmf" else "g8"
    sfx = "_full" if arch == "cmf" else ""
    left, right = seeded(f"{tag}.left{sfx}", 1, 3, 256, 512).cuda(), seeded(f"{tag}.right{sfx}", 1, 3, 256, 512).cuda()
    ref = None
    if arch in ("cmfsm", "cmf"):             # fp64 fixtures of these weights and inputs (g8d, g13), every 4th pixel
        z = _z("g8d_full_cmfsm_256x512_fp64" if arch == "cmfsm" else "g13_full_cmf_256x512_fp64")
        ref = [torch.from_numpy(z[f"o{i}_64"]).reshape(1, *z[f"o{i}_64"].shape[-2:]) for i in (1, 2, 3)]
    _accuracy(ecm, arch, left, right, ref, sub=4 if ref is not None else 1)


def test_cmfsm_accuracy_576x960(ecm):
    from oracle.weights import fullframe_frame
    z = _z("g12_full_cmfsm_576x960_fp64")
    frame = torch.from_numpy(fullframe_frame("sceneflow")[None].copy()).cuda()
    left, right, _ = ecm.ops.frame_prep(frame, [0], [0], 576, 960, split=540, tail=36)
    ref = [torch.from_numpy(z[f"o{i}_64"]).reshape(1, *z[f"o{i}_64"].shape[-2:]) for i in (1, 2, 3)]
    _accuracy(ecm, "cmfsm", left, right, ref, sub=4)


def test_cmfsm_accuracy_384x1248(ecm):
    from oracle.weights import fullframe_frame
    z = _z("g12k_full_cmfsm_384x1248_fp64")
    frame = torch.from_numpy(fullframe_frame("kitti")[None].copy()).cuda()
    left, right, _ = ecm.ops.frame_prep_kitti_eval(frame, 384, 1248)
    ref = [torch.from_numpy(z[f"o{i}_64"]).reshape(1, *z[f"o{i}_64"].shape[-2:]) for i in (1, 2, 3)]
    _accuracy(ecm, "cmfsm", left, right, ref, sub=4)


def test_encoder_results_are_fp32(ecm):
    for variant in ("cmfsm", "sub8", "cmf"):
        fe = ecm.models.feature_extraction(variant).cuda().eval()
        x = seeded("er.x", 2, 3, 256, 512).cuda()
        with torch.no_grad(), ecm.ops.encoder_dtype(BF):
            lr, rt, hr = fe(x, head=1)
        with torch.no_grad():
            lr32, rt32, hr32 = fe(x, head=1)
        for a, b in ((lr, lr32), (rt, rt32), (hr, hr32)):
            assert a.dtype == torch.float32 and a.shape == b.shape, variant
            assert float((a - b).abs().max()) <= 0.1 * float(b.abs().max()) + 1e-3, variant


def test_fp32_unaffected_by_bf16_block(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("fp.left", 1, 3, 256, 512).cuda(), seeded("fp.right", 1, 3, 256, 512).cuda()
    for ctx in (contextlib.nullcontext, ecm.ops.frozen_weights):
        with ctx():
            a = _run(ecm, model, left, right, "fp32")
            _run(ecm, model, left, right, "enc")
            _run(ecm, model, left, right, "both")
            b = _run(ecm, model, left, right, "fp32")
        assert all(torch.equal(x, y) for x, y in zip(a, b)), ctx


def test_frozen_weights_caches_bf16_images(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("fw.left", 1, 3, 256, 512).cuda(), seeded("fw.right", 1, 3, 256, 512).cuda()
    plain = _run(ecm, model, left, right, "enc")
    with ecm.ops.frozen_weights():
        a = _run(ecm, model, left, right, "enc")
        w = model.feature_extraction.layer3[0].conv1[0][0].weight
        assert "bf16_conv2d" in w._ecm_packed
        cached = w._ecm_packed["bf16_conv2d"][1]
        b = _run(ecm, model, left, right, "enc")
        assert w._ecm_packed["bf16_conv2d"][1] is cached
        ecm.ops.invalidate_packed()
        c = _run(ecm, model, left, right, "enc")
        assert w._ecm_packed["bf16_conv2d"][1] is not cached
    assert all(torch.equal(x, y) and torch.equal(x, u) and torch.equal(x, v) for x, y, u, v in zip(plain, a, b, c))


def test_grad_enabled_forward_raises_before_any_encoder_launch(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("gr.left", 1, 3, 256, 512).cuda(), seeded("gr.right", 1, 3, 256, 512).cuda()
    before = _run(ecm, model, left, right, "fp32")
    calls = []
    real_call = ecm._lib.call

    def rec(name, *args):
        calls.append(name)
        return real_call(name, *args)
    ecm._lib.call = rec
    try:
        with ecm.ops.encoder_dtype(BF), pytest.raises(RuntimeError, match="no backward"):
            model(left, right)
    finally:
        ecm._lib.call = real_call
    assert calls == [], calls                    # frame glue aside, the encoder is the first thing the model launches
    after = _run(ecm, model, left, right, "fp32")
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_bf16_forward_is_bit_reproducible(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("rp.left", 2, 3, 256, 512).cuda(), seeded("rp.right", 2, 3, 256, 512).cuda()
    for mode in ("enc", "both"):
        a = _run(ecm, model, left, right, mode)
        b = _run(ecm, model, left, right, mode)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), mode


@pytest.mark.parametrize("hw", [(576, 960), (384, 1248)])
def test_no_slow_path_bf16_encoder(ecm, hw):
    """No slow-path event in bf16 mode, for every architecture the fp32 model accepts -- not even the fp32 encoder's
    `dilated_stage_unphased` note: the bf16 kernel runs the dilation natively."""
    ran = []
    for arch in ARCHS:
        if not _fp32_accepts(arch, hw):
            continue
        model = _model(ecm, arch)
        left, right = seeded("sp.left", 1, 3, *hw).cuda(), seeded("sp.right", 1, 3, *hw).cuda()
        for mode in ("enc", "both"):
            ecm.models.SLOW_PATH_EVENTS.clear()
            o = _run(ecm, model, left, right, mode)
            assert ecm.models.SLOW_PATH_EVENTS == [], (arch, mode, ecm.models.SLOW_PATH_EVENTS)
            assert all(tuple(t.shape[-2:]) == hw and bool(torch.isfinite(t).all()) for t in o), (arch, mode)
        ran.append(arch)
        del model
    assert len(ran) >= 7, ran


def test_data_parallel_takes_bf16_encoder_path(ecm):
    model = _model(ecm, "cmfsm")
    dp = torch.nn.DataParallel(model, device_ids=[0])
    left, right = seeded("dp.left", 1, 3, 256, 512).cuda(), seeded("dp.right", 1, 3, 256, 512).cuda()
    a = _run(ecm, model, left, right, "enc")
    b = _run(ecm, dp, left, right, "enc")
    f = _run(ecm, model, left, right, "fp32")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a, f))       # it did take the bf16 path


def test_encoder_bf16_eval_faster_b4_576x960(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("tm.left", 4, 3, 576, 960).cuda(), seeded("tm.right", 4, 3, 576, 960).cuda()

    def ms(enc):
        with torch.no_grad(), ecm.ops.frozen_weights(), ecm.ops.aggregation_dtype(BF), \
                (ecm.ops.encoder_dtype(BF) if enc else contextlib.nullcontext()):
            for _ in range(2):
                model(left, right)
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                model(left, right)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2] * 1e3
    agg, both = ms(False), ms(True)
    print(f"cmfsm eval B=4 576x960: aggregation-only bf16 {agg:.2f} ms, encoder + aggregation bf16 {both:.2f} ms, "
          f"ratio {agg / both:.2f}")
    assert both < agg, (agg, both)
