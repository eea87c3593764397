"""The opt-in bf16 aggregation stack (ops.aggregation_dtype) on the MI355X.

Kernel parity: every new kernel against the fp32 computation of the same bf16-rounded operands (F.conv3d / F.conv_transpose3d /
F.group_norm in fp32 on MIOpen), within 1 bf16 ulp of that yardstick rounded to bf16 (or 1e-5 of the output's max |value| where
cancellation makes a value tiny).  Whole models: the HIP bf16 disparities against a reference R (the fp64 fixtures where they
exist, else the unmodified fp32 HIP output) within 2x the mean and 4x the max distance of an EMULATION -- the library's own
fp32 path with bf16 rounding injected at exactly the new kernels' rounding points.

The per-path numerical check of these kernels (every instantiation against fp64, once-rounded outputs, repeats on poisoned
memory) is tests/test_hip_bf16_fp64.py with tests/test_bf16_geometry.py; the bars below are kept as they were."""
import contextlib
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from oracle.weights import seeded, tensor_for
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ARCHS = ("cmfsm", "cmfsm_sub_8", "cmfsm_sub_16", "cm_sub_4", "cm_sub_8", "cm_sub_16", "bilinear_cmf", "bilinear_cmf_sub_8",
         "bilinear_cmf_sub_16", "cmf")
SCALE = {"cmfsm": 4, "cmf": 4, "cm_sub_4": 4, "bilinear_cmf": 4, "cmfsm_sub_8": 8, "cm_sub_8": 8, "bilinear_cmf_sub_8": 8,
         "cmfsm_sub_16": 16, "cm_sub_16": 16, "bilinear_cmf_sub_16": 16}


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def _R(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


def _within_ulp(got, want32, label):
    """got (bf16) within 1 bf16 ulp of the fp32 yardstick rounded to bf16, or 1e-5 x max|want| where values are tiny."""
    want = want32.to(BF).float()
    g = got.float()
    mag = torch.maximum(want.abs(), g.abs())
    ulp = torch.exp2(torch.floor(torch.log2(mag.clamp_min(1e-38))) - 7)
    tol = torch.maximum(ulp, torch.full_like(ulp, 1e-5 * float(want32.abs().max())))
    err = (g - want).abs()
    bad = int((err > tol).sum())
    assert bad == 0, f"{label}: {bad} of {g.numel()} elements off by more than 1 bf16 ulp (worst {float((err / tol).max()):.2f} ulp)"
    assert torch.isfinite(g).all(), label


# ------------------------------------------------------------------------------------------------ kernel parity
# (B, Ci, Co, (D, H, W), stride): the stack's layers at 576x960 (D' = 48) and its 1/2 and 1/4 hourglass levels, plus awkward
# shapes (w = 78: rows of 156 bytes, D' = 12, batch 1, odd sizes after a stride-2 layer; stride 2 onto one output-channel tile,
# eight chunks, odd extents)
_CONV = [(4, 32, 32, (48, 144, 240), 1), (4, 32, 64, (48, 144, 240), 2), (4, 64, 64, (24, 72, 120), 1),
         (4, 64, 64, (24, 72, 120), 2), (4, 64, 64, (12, 36, 60), 1),
         (1, 32, 32, (12, 24, 78), 1), (1, 32, 64, (12, 24, 78), 2), (1, 64, 64, (6, 12, 39), 1), (1, 64, 64, (6, 12, 39), 2),
         (2, 32, 32, (3, 5, 33), 1), (1, 64, 64, (1, 1, 1), 2), (1, 64, 32, (3, 5, 35), 2)]


@pytest.mark.parametrize("B,Ci,Co,dims,stride", _CONV)
def test_conv3d_bf16_parity(ecm, B, Ci, Co, dims, stride):
    x = _R(B, Ci, *dims, seed=1, dtype=BF)
    w = _R(Co, Ci, 3, 3, 3, seed=2, scale=(2.0 / (27 * Co)) ** 0.5)
    with torch.no_grad():
        y = ecm.ops.conv3d_k3(x, w, stride)
        want = F.conv3d(x.float(), w.bfloat16().float(), stride=stride, padding=1)
    assert y.dtype == BF and y.shape == want.shape and y.is_contiguous()
    _within_ulp(y, want, f"conv3d {B}x{Ci}->{Co} {dims} s{stride}")


_DECONV = [(4, 64, 64, (12, 36, 60)), (4, 64, 32, (24, 72, 120)), (1, 64, 32, (6, 12, 39)), (1, 64, 64, (3, 6, 20)),
           (2, 64, 32, (1, 3, 5))]


@pytest.mark.parametrize("B,Ci,Co,dims", _DECONV)
def test_deconv3d_bf16_parity(ecm, B, Ci, Co, dims):
    x = _R(B, Ci, *dims, seed=3, dtype=BF)
    w = _R(Ci, Co, 3, 3, 3, seed=4, scale=(2.0 / (27 * Co)) ** 0.5)
    with torch.no_grad():
        y = ecm.ops.deconv3d_k3s2(x, w)
        want = F.conv_transpose3d(x.float(), w.bfloat16().float(), stride=2, padding=1, output_padding=1)
    assert y.dtype == BF and y.shape == want.shape
    _within_ulp(y, want, f"deconv3d {B}x{Ci}->{Co} {dims}")


_GN = [(4, 32, (48, 144, 240)), (4, 64, (24, 72, 120)), (4, 64, (12, 36, 60)), (1, 32, (12, 24, 78)), (1, 64, (3, 6, 39)),
       (2, 32, (1, 1, 3))]


@pytest.mark.parametrize("B,Cc,dims", _GN)
@pytest.mark.parametrize("mode", ["bf16", "bf16_skip_relu", "f32_in", "f32_in_skip"])
def test_group_norm_bf16_parity(ecm, B, Cc, dims, mode):
    f32_in = mode.startswith("f32")
    x = _R(B, Cc, *dims, seed=5, scale=3.0)
    x = x + 2.0                                           # |mean| > 0: the variance formulation matters
    if not f32_in:
        x = x.to(BF)
    skip = _R(B, Cc, *dims, seed=6, dtype=BF) if "skip" in mode else None
    relu = "relu" in mode or mode == "f32_in"
    g, b = _R(Cc, seed=7, scale=0.5) + 1.0, _R(Cc, seed=8, scale=0.5)
    with torch.no_grad():
        y = ecm.ops.group_norm_act(x, g, b, skip, relu, out_dtype=BF)
        want = F.group_norm(x.float(), 32, g, b, eps=1e-5)
        if skip is not None:
            want = want + skip.float()
        if relu:
            want = want.clamp_min(0)
    assert y.dtype == BF
    _within_ulp(y, want, f"group_norm {mode} {B}x{Cc} {dims}")


@pytest.mark.parametrize("B,dims", [(4, (48, 144, 240)), (1, (12, 24, 78)), (2, (3, 5, 9))])
def test_classifier_tail_bf16_parity(ecm, B, dims):
    x = _R(B, 32, *dims, seed=9, scale=2.0, dtype=BF)
    g, b = _R(32, seed=10, scale=0.5) + 1.0, _R(32, seed=11, scale=0.5)
    w = _R(1, 32, 3, 3, 3, seed=12, scale=0.1)
    with torch.no_grad():
        y = ecm.ops.classifier_tail(x, g, b, w)
        h = F.group_norm(x.float(), 32, g, b, eps=1e-5).clamp_min(0)
        want = F.conv3d(h, w, padding=1)
    assert y.dtype == torch.float32 and y.shape == want.shape
    err = (y - want).abs()
    tol = 2e-5 * float(want.abs().max()) + 1e-4 * want.abs()     # fp32 accumulation order (864 terms)
    assert bool((err <= tol).all()), float((err - tol).max())


def test_bf16_conv_outside_contract_raises(ecm):
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="Ci, Co in"):
            ecm.ops.conv3d_k3(_R(1, 16, 2, 2, 4, dtype=BF), _R(16, 16, 3, 3, 3))
        with pytest.raises(RuntimeError, match="Ci, Co in"):
            ecm.ops.deconv3d_k3s2(_R(1, 64, 2, 2, 4, dtype=BF), _R(64, 48, 3, 3, 3))


def test_f32_to_bf16_keeps_nan(ecm):
    x = _R(1, 32, 2, 3, 8, seed=13)
    x[0, 0, 0, 0, 0] = float("nan")
    with torch.no_grad():
        y = ecm.ops.group_norm_act(x, torch.ones(32, device="cuda"), torch.zeros(32, device="cuda"), out_dtype=BF)
    assert bool(torch.isnan(y[0, 0]).all())                 # the NaN poisons its group's statistics, and stays NaN
    assert bool(torch.isfinite(y[0, 1:]).all())


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B,Ci,Co,dims,stride", [(1, 32, 32, (3, 5, 78), 1), (1, 32, 64, (5, 7, 39), 2), (2, 64, 64, (2, 3, 33), 2),
                                                 (1, 64, 32, (3, 5, 35), 2)])
def test_guard_bands_conv3d_bf16(ecm, B, Ci, Co, dims, stride):
    x, w = _R(B, Ci, *dims, seed=1, dtype=BF), _R(Co, Ci, 3, 3, 3, seed=2, scale=0.1)
    with torch.no_grad(), guarded(ecm) as g:
        ecm.ops.conv3d_k3(x, w, stride)
        g.check(f"conv3d bf16 {B}x{Ci}->{Co} {dims} s{stride}")


@pytest.mark.parametrize("B,Ci,Co,dims", [(1, 64, 32, (3, 5, 39)), (2, 64, 64, (1, 2, 33))])
def test_guard_bands_deconv3d_bf16(ecm, B, Ci, Co, dims):
    x, w = _R(B, Ci, *dims, seed=1, dtype=BF), _R(Ci, Co, 3, 3, 3, seed=2, scale=0.1)
    with torch.no_grad(), guarded(ecm) as g:
        ecm.ops.deconv3d_k3s2(x, w)
        g.check(f"deconv3d bf16 {B}x{Ci}->{Co} {dims}")


@pytest.mark.parametrize("dims", [(3, 5, 78), (1, 1, 3), (2, 4, 8)])
def test_guard_bands_group_norm_and_tail_bf16(ecm, dims):
    g32, b32 = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    with torch.no_grad(), guarded(ecm) as g:
        x = _R(2, 32, *dims, seed=1)
        h = ecm.ops.group_norm_act(x, g32, b32, None, True, out_dtype=BF)
        h = ecm.ops.group_norm_act(h, g32, b32, h, True)
        ecm.ops.classifier_tail(h, g32, b32, _R(1, 32, 3, 3, 3, seed=3))
        g.check(f"group_norm / tail bf16 {dims}")


# ------------------------------------------------------------------------------------------------ whole models
def _model(ecm, arch):
    m = ecm.get_model(arch)
    m.load_state_dict({k: tensor_for(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().eval()


@contextlib.contextmanager
def _emulated(ecm):
    """The fp32 path with bf16 rounding at the new kernels' rounding points: convolution inputs, weights and outputs,
    GroupNorm outputs (skips are GroupNorm outputs already), the classifier tail's input.  GroupNorms are rounded from the
    cost volume on (the encoder's dilated stages run GroupNorm on 5-D phase planes too)."""
    ops = ecm.ops
    r = lambda t: t.to(BF).float()
    conv, deconv, gn, tail = ops.conv3d_k3, ops.deconv3d_k3s2, ops.group_norm_act, ops.classifier_tail
    cv, cvx = ops.costvol_conv3d, ops.cost_volume
    region = [False]

    def cv_e(*a):
        region[0] = True
        return cv(*a)

    def cvx_e(*a):
        region[0] = True
        return cvx(*a)

    def conv_e(x, w, stride=1, fork=False):
        out = conv(r(x), r(w), stride, fork)
        return (r(out[0]), out[1]) if fork else r(out)

    def gn_e(x, gamma, beta, skip=None, relu=False, head=0, out_dtype=None):
        y = gn(x, gamma, beta, skip, relu, head)
        return r(y) if region[0] and x.dim() == 5 else y

    ops.conv3d_k3 = conv_e
    ops.deconv3d_k3s2 = lambda x, w: r(deconv(r(x), r(w)))
    ops.group_norm_act = gn_e
    ops.classifier_tail = lambda x, gamma, beta, w: tail(r(x), gamma, beta, w)
    ops.costvol_conv3d, ops.cost_volume = cv_e, cvx_e
    try:
        yield
    finally:
        ops.conv3d_k3, ops.deconv3d_k3s2, ops.group_norm_act, ops.classifier_tail = conv, deconv, gn, tail
        ops.costvol_conv3d, ops.cost_volume = cv, cvx


def _run(ecm, model, left, right, mode):
    with torch.no_grad():
        if mode == "bf16":
            with ecm.ops.aggregation_dtype(BF):
                o = model(left, right)
        elif mode == "emu":
            with _emulated(ecm):
                o = model(left, right)
        else:
            o = model(left, right)
    torch.cuda.synchronize()
    return [t.detach().double().cpu().reshape(-1, *t.shape[-2:]) for t in o]


def _z(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _accuracy(ecm, arch, left, right, ref=None, sub=1):
    """-> per head (E_mean, E_max, bf16 mean, bf16 max); asserts the 2x / 4x bar against R."""
    model = _model(ecm, arch)
    if ref is None:
        ref = _run(ecm, model, left, right, "fp32")
    emu = _run(ecm, model, left, right, "emu")
    b16 = _run(ecm, model, left, right, "bf16")
    rows = []
    for i, (r, e, b) in enumerate(zip(ref, emu, b16)):
        e, b = e[..., ::sub, ::sub], b[..., ::sub, ::sub]
        de, db = (e - r).abs(), (b - r).abs()
        row = (float(de.mean()), float(de.max()), float(db.mean()), float(db.max()))
        print(f"{arch} {tuple(left.shape[-2:])} head {i + 1}: E_mean {row[0]:.3e} E_max {row[1]:.3e} | bf16 mean {row[2]:.3e} "
              f"max {row[3]:.3e}")
        assert row[2] <= 2 * row[0] and row[3] <= 4 * row[1], (arch, i, row)
        rows.append(row)
    return rows


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


def test_fp32_unaffected_by_bf16_block(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("fp.left", 1, 3, 256, 512).cuda(), seeded("fp.right", 1, 3, 256, 512).cuda()
    for ctx in (contextlib.nullcontext, ecm.ops.frozen_weights):
        with ctx():
            a = _run(ecm, model, left, right, "fp32")
            _run(ecm, model, left, right, "bf16")
            b = _run(ecm, model, left, right, "fp32")
        assert all(torch.equal(x, y) for x, y in zip(a, b)), ctx


def test_frozen_weights_caches_bf16_images(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("fw.left", 1, 3, 256, 512).cuda(), seeded("fw.right", 1, 3, 256, 512).cuda()
    plain = _run(ecm, model, left, right, "bf16")
    with ecm.ops.frozen_weights():
        a = _run(ecm, model, left, right, "bf16")
        w = model.dres2.conv1[0][0].weight
        assert "bf16_conv" in w._ecm_packed
        b = _run(ecm, model, left, right, "bf16")
        ecm.ops.invalidate_packed()
        c = _run(ecm, model, left, right, "bf16")
    assert all(torch.equal(x, y) and torch.equal(x, u) and torch.equal(x, v) for x, y, u, v in zip(plain, a, b, c))


def test_grad_enabled_forward_raises_before_any_3d_launch(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("gr.left", 1, 3, 256, 512).cuda(), seeded("gr.right", 1, 3, 256, 512).cuda()
    before = _run(ecm, model, left, right, "fp32")
    calls, state = [], {"enc": False}
    real_call, real_fe = ecm._lib.call, model.feature_extraction.forward

    def rec(name, *args):
        if state["enc"]:
            calls.append(name)
        return real_call(name, *args)

    def fe(*a, **k):
        out = real_fe(*a, **k)
        state["enc"] = True
        return out
    ecm._lib.call = rec
    model.feature_extraction.forward = fe
    try:
        with ecm.ops.aggregation_dtype(BF), pytest.raises(RuntimeError, match="no backward"):
            model(left, right)
    finally:
        ecm._lib.call = real_call
        del model.feature_extraction.forward
    assert state["enc"]
    assert set(calls) <= {"ecm_weights9_fwd"}, calls            # the ECM weights (2-D) precede the cost volume; no 3-D op ran
    after = _run(ecm, model, left, right, "fp32")
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_bf16_forward_is_bit_reproducible(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("rp.left", 2, 3, 256, 512).cuda(), seeded("rp.right", 2, 3, 256, 512).cuda()
    a = _run(ecm, model, left, right, "bf16")
    b = _run(ecm, model, left, right, "bf16")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _fp32_accepts(arch, hw):
    """The hourglass halves the 1/s volume twice and doubles it back: the fp32 model takes sizes divisible by 4 there."""
    h, w = hw[0] // SCALE[arch], hw[1] // SCALE[arch]
    return h % 4 == 0 and w % 4 == 0


@pytest.mark.parametrize("hw", [(576, 960), (384, 1248)])
def test_no_slow_path_bf16(ecm, hw):
    """The bf16 region adds no slow-path event: every architecture's bf16 forward records exactly what its fp32 forward does --
    nothing, except the fp32 ENCODER's own note where a dilated stage's map does not split into phase planes (the 1/8 nets'
    layer at these sizes), which is outside the bf16 region and unchanged by it."""
    ran = []
    for arch in ARCHS:
        if not _fp32_accepts(arch, hw):
            continue
        model = _model(ecm, arch)
        left, right = seeded("sp.left", 1, 3, *hw).cuda(), seeded("sp.right", 1, 3, *hw).cuda()
        ecm.models.SLOW_PATH_EVENTS.clear()
        _run(ecm, model, left, right, "fp32")
        ev32 = list(ecm.models.SLOW_PATH_EVENTS)
        ecm.models.SLOW_PATH_EVENTS.clear()
        o = _run(ecm, model, left, right, "bf16")
        assert ecm.models.SLOW_PATH_EVENTS == ev32, (arch, ecm.models.SLOW_PATH_EVENTS, ev32)
        assert all(kind == "dilated_stage_unphased" for kind, *_ in ev32), (arch, ev32)
        if arch in ("cmfsm", "cmf"):
            assert ev32 == [], (arch, ev32)
        ecm.models.SLOW_PATH_EVENTS.clear()
        assert all(tuple(t.shape[-2:]) == hw and bool(torch.isfinite(t).all()) for t in o), arch
        ran.append(arch)
        del model
    assert len(ran) >= 7, ran


def test_data_parallel_takes_bf16_path(ecm):
    model = _model(ecm, "cmfsm")
    dp = torch.nn.DataParallel(model, device_ids=[0])
    left, right = seeded("dp.left", 1, 3, 256, 512).cuda(), seeded("dp.right", 1, 3, 256, 512).cuda()
    a = _run(ecm, model, left, right, "bf16")
    b = _run(ecm, dp, left, right, "bf16")
    f = _run(ecm, model, left, right, "fp32")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a, f))       # it did take the bf16 path


def test_bf16_eval_faster_than_fp32_b4_576x960(ecm):
    model = _model(ecm, "cmfsm")
    left, right = seeded("tm.left", 4, 3, 576, 960).cuda(), seeded("tm.right", 4, 3, 576, 960).cuda()

    def ms(bf16):
        ctx = ecm.ops.aggregation_dtype(BF) if bf16 else contextlib.nullcontext()
        with torch.no_grad(), ecm.ops.frozen_weights(), ctx:
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
    f32, b16 = ms(False), ms(True)
    print(f"cmfsm eval B=4 576x960: fp32 {f32:.1f} ms, bf16 {b16:.1f} ms, ratio {f32 / b16:.2f}")
    assert b16 < f32, (f32, b16)
