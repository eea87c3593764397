"""The opt-in bf16 refinement decoder (ops.decoder_dtype, ops.inference_dtype) on the MI355X.

Kernel parity: the bf16 transposed convolution against F.conv_transpose2d and the bf16-input conv_out against F.conv2d + relu,
both in fp32 on the same bf16-rounded operands -- bf16 outputs within 1 bf16 ulp of that yardstick rounded to bf16 (or 1e-5 of
max |y| where a value is tiny), fp32 outputs within fp32 accumulation-order tolerance.  Decoder and whole model: the bf16
disparities against the fp64 fixtures within 2x the mean and 4x the max distance of an EMULATION: the decoder's own bf16
forward with every bf16 kernel replaced by the library's fp32 kernel on the same bf16 values, rounded where the bf16 kernel
rounds.

The per-path numerical check of these kernels (every instantiation against fp64, once-rounded outputs, repeats on poisoned
memory) is tests/test_hip_bf16_fp64.py with tests/test_bf16_geometry.py; the bars below are kept as they were."""
import contextlib
import time

import pytest
import torch
import torch.nn.functional as F

from oracle.weights import seeded, tensor_for
from test_hip_bf16_encoder import _R, _enc_emulated, _within_f32
from test_hip_bf16_infer import ARCHS, _emulated, _model, _within_ulp, _z
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


# ------------------------------------------------------------------------------------------------ kernel A parity
# (B, Ci, Co, H, W): one position; less than a tile; exactly one tile of 4 x 32 inputs; one past it in both directions; several
# tiles with a ragged edge (w = 78: rows that are not 16-byte aligned); Co = 32; a single 16-channel chunk; the decoder's first
# level at B = 1 (3 heads) and at B = 4 (12 images); Co = 32 with 2-byte row loads at two chunks and 16-byte ones at three
_DECONV = [(1, 96, 64, 1, 1), (2, 96, 64, 3, 5), (1, 96, 64, 4, 32), (1, 96, 64, 8, 32), (1, 96, 64, 9, 33), (1, 96, 64, 5, 33),
           (2, 96, 64, 17, 78), (1, 32, 32, 5, 40), (1, 16, 64, 4, 7), (3, 96, 64, 36, 60), (12, 96, 64, 144, 240),
           (1, 32, 32, 5, 33), (1, 48, 32, 4, 40)]


def _deconv_case(ecm, B, Ci, Co, H, W, bias):
    x = _R(B, Ci, H, W, seed=1, dtype=BF)
    w = _R(Ci, Co, 3, 3, seed=2, scale=(2.0 / (9 * Co)) ** 0.5)
    with torch.no_grad(), torch.backends.cudnn.flags(allow_tf32=False):
        y = ecm.ops.deconv2d_k3s2_bias_bf16(x, w, bias)
        want = F.conv_transpose2d(x.float(), w.bfloat16().float(), bias, stride=2, padding=1, output_padding=1)
    assert y.dtype == BF and y.shape == want.shape == (B, Co, 2 * H, 2 * W) and y.is_contiguous()
    _within_ulp(y, want, f"deconv2d {B}x{Ci}->{Co} {H}x{W}")


@pytest.mark.parametrize("B,Ci,Co,H,W", _DECONV)
def test_deconv2d_bf16_parity(ecm, B, Ci, Co, H, W):
    _deconv_case(ecm, B, Ci, Co, H, W, _R(Co, seed=3, scale=0.5))


@pytest.mark.parametrize("bias", ["zero", "large"])
def test_deconv2d_bf16_bias_joins_the_accumulator(ecm, bias):
    """A bias of +-50 added after the rounding (two roundings per output) would miss the 1-ulp bar."""
    b = torch.zeros(64, device="cuda") if bias == "zero" else 50.0 * torch.sign(_R(64, seed=4))
    _deconv_case(ecm, 2, 96, 64, 9, 33, b)


def test_deconv2d_bf16_keeps_nan(ecm):
    """One NaN input reaches exactly the up-to-3x3 outputs that read it -- in all four phases -- and nothing else."""
    x = _R(1, 32, 4, 40, seed=9, dtype=BF)
    x[0, 0, 1, 5] = float("nan")
    with torch.no_grad():
        y = ecm.ops.deconv2d_k3s2_bias_bf16(x, _R(32, 64, 3, 3, seed=10, scale=0.1), _R(64, seed=11))
    hit = torch.zeros(8, 80, dtype=torch.bool, device="cuda")
    hit[1:4, 9:12] = True
    nan = torch.isnan(y[0])
    assert bool((nan == hit.expand_as(nan)).all())
    assert bool(torch.isfinite(y[0][:, ~hit]).all())


# ------------------------------------------------------------------------------------------------ kernel B parity
_C1 = [(1, 96, 1, 1), (2, 96, 3, 5), (1, 96, 9, 33), (2, 96, 17, 78), (1, 16, 5, 40), (1, 32, 8, 64), (1, 96, 17, 520),
       (1, 96, 5, 1024), (12, 96, 576, 960)]


@pytest.mark.parametrize("B,Ci,H,W", _C1)
def test_conv2d_c1_bf16_parity(ecm, B, Ci, H, W):
    """fp32 out; the bias sits near the median of the sums, so the ReLU is exercised on both sides.  (W = 520 and 1024: the
    column blocks of 512 that a wave covers, ragged and exact, beyond what the issue lists.)"""
    x = _R(B, Ci, H, W, seed=5, dtype=BF)
    w = _R(1, Ci, 3, 3, seed=6, scale=(2.0 / 9) ** 0.5)
    b = torch.full((1,), 0.05, device="cuda")
    with torch.no_grad(), torch.backends.cudnn.flags(allow_tf32=False):
        y = ecm.ops.conv2d_c1_relu_bf16(x, w, b)
        want = F.relu(F.conv2d(x.float(), w.bfloat16().float(), b, padding=1))
    assert y.dtype == torch.float32 and y.shape == want.shape == (B, 1, H, W) and y.is_contiguous()
    if y.numel() >= 64:
        frac = float((want == 0).float().mean())
        assert 0.25 < frac < 0.75, frac
    _within_f32(y, want, f"conv_out {B}x{Ci} {H}x{W}")


def test_outside_contract_raises(ecm):
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="Ci % 16"):
            ecm.ops.deconv2d_k3s2_bias_bf16(_R(1, 24, 4, 8, dtype=BF), _R(24, 64, 3, 3), _R(64))
        with pytest.raises(RuntimeError, match="Co in"):
            ecm.ops.deconv2d_k3s2_bias_bf16(_R(1, 96, 4, 8, dtype=BF), _R(96, 48, 3, 3), _R(48))
        with pytest.raises(RuntimeError, match="Ci % 16"):
            ecm.ops.conv2d_c1_relu_bf16(_R(1, 24, 4, 8, dtype=BF), _R(1, 24, 3, 3), _R(1))


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B,Ci,Co,H,W", [(1, 96, 64, 5, 33), (2, 32, 32, 1, 1), (1, 32, 32, 5, 33)])
def test_guard_bands_deconv2d_bf16(ecm, B, Ci, Co, H, W):
    x, w, b = _R(B, Ci, H, W, seed=1, dtype=BF), _R(Ci, Co, 3, 3, seed=2, scale=0.1), _R(Co, seed=3)
    with torch.no_grad(), guarded(ecm) as g:
        ecm.ops.deconv2d_k3s2_bias_bf16(x, w, b)                                   # the pack's image is guarded too
        g.check(f"deconv2d bf16 {B}x{Ci}->{Co} {H}x{W}")
        assert len(g.records) >= 2


@pytest.mark.parametrize("B,Ci,H,W", [(1, 96, 5, 78), (2, 16, 1, 1)])
def test_guard_bands_conv2d_c1_bf16(ecm, B, Ci, H, W):
    x, w, b = _R(B, Ci, H, W, seed=1, dtype=BF), _R(1, Ci, 3, 3, seed=2, scale=0.1), _R(1, seed=3)
    with torch.no_grad(), guarded(ecm) as g:
        ecm.ops.conv2d_c1_relu_bf16(x, w, b)
        g.check(f"conv_out bf16 {B}x{Ci} {H}x{W}")


# ------------------------------------------------------------------------------------------------ decoder and whole model
@contextlib.contextmanager
def _dec_emulated(ecm):
    """The bf16 decoder's own forward (models.super_resolution_refinement._forward_bf16: same rounding points, bf16 tensors
    between layers) with every bf16 kernel replaced by the library's fp32 kernel on the same bf16 values: a convolution or
    transposed convolution computes in fp32 on the rounded input and weights (fp32 bias) and rounds its output once; a
    GroupNorm computes in fp32 and rounds its output once; conv_out computes in fp32 and rounds nothing."""
    ops = ecm.ops
    r = lambda t: t.to(BF).float()
    conv_bf, gn, dcv, c1 = ops.conv2d_bf16, ops.group_norm_act, ops.deconv2d_k3s2_bias_bf16, ops.conv2d_c1_relu_bf16
    with _enc_emulated(ecm):                    # the convolution and GroupNorm wrappers ARE the encoder emulation's: one rule
        conv_e, gn_e = ops.conv2d_bf16, ops.group_norm_act

    ops.conv2d_bf16, ops.group_norm_act = conv_e, gn_e
    ops.deconv2d_k3s2_bias_bf16 = lambda x, w, b: ops.deconv2d_k3s2_bias(x.float(), r(w), b).to(BF)
    ops.conv2d_c1_relu_bf16 = lambda x, w, b: ops.conv2d_c1_relu(x.float(), r(w), b)
    try:
        with ops.decoder_dtype(BF):
            yield
    finally:
        ops.conv2d_bf16, ops.group_norm_act, ops.deconv2d_k3s2_bias_bf16, ops.conv2d_c1_relu_bf16 = conv_bf, gn, dcv, c1


def _bar(label, ref, emu, b16):
    de, db = (emu - ref).abs(), (b16 - ref).abs()
    row = (float(de.mean()), float(de.max()), float(db.mean()), float(db.max()))
    print(f"{label}: E_mean {row[0]:.3e} E_max {row[1]:.3e} | bf16 mean {row[2]:.3e} max {row[3]:.3e}")
    assert row[2] <= 2 * row[0] and row[3] <= 4 * row[1], (label, row)


def test_decoder_alone_against_fp64_reference(ecm):
    """super_resolution_refinement alone on the g13 fixture (B = 2, 8x16 -> 32x64): fp32, bf16 and the emulation vs fp64."""
    z = _z("g13_srr_decoder")
    srr = ecm.super_resolution_refinement(32, 2)
    srr.load_state_dict({k: tensor_for("srr." + k, v.shape) for k, v in srr.state_dict().items()})
    srr = srr.cuda().eval()
    B, h, w = 2, 8, 16
    ins = (seeded("g13.pred", B, h, w).abs().mul(8.0).unsqueeze(0).cuda(), seeded("g13.left", B, 3, 4 * h, 4 * w).cuda(),
           seeded("g13.ref", B, 32, h, w).cuda(), seeded("g13.half", B, 32, 2 * h, 2 * w).cuda())
    ref = torch.from_numpy(z["y_64"]).reshape(B, 4 * h, 4 * w)
    out = {}
    with torch.no_grad():
        out["fp32"] = srr(*ins)
        with ecm.ops.decoder_dtype(BF):
            out["bf16"] = srr(*ins)
        with _dec_emulated(ecm):
            out["emu"] = srr(*ins)
    ecm.ops.check_async_errors()
    for k, v in out.items():
        assert v.dtype == torch.float32 and tuple(v.shape) == (1, B, 1, 4 * h, 4 * w), k
    o = {k: v.double().cpu().reshape(B, 4 * h, 4 * w) for k, v in out.items()}
    print(f"decoder fp32 vs fp64: mean {float((o['fp32'] - ref).abs().mean()):.3e} max {float((o['fp32'] - ref).abs().max()):.3e}")
    assert not torch.equal(o["bf16"], o["fp32"])                     # the bf16 path was taken
    _bar("decoder alone", ref, o["emu"], o["bf16"])


def _run(ecm, model, left, right, mode):
    """mode: fp32 | enc | agg | dec | all | dec_emu | all_emu"""
    ops = ecm.ops
    with torch.no_grad(), contextlib.ExitStack() as st:
        if mode == "all_emu":
            st.enter_context(_emulated(ecm))
            st.enter_context(_enc_emulated(ecm))     # inside the aggregation emulation: its GroupNorm wrapper sees fp32
        if mode.endswith("emu"):
            st.enter_context(_dec_emulated(ecm))
        elif mode == "all":
            st.enter_context(ops.inference_dtype(BF))
        elif mode != "fp32":
            st.enter_context({"enc": ops.encoder_dtype, "agg": ops.aggregation_dtype, "dec": ops.decoder_dtype}[mode](BF))
        o = model(left, right)
    torch.cuda.synchronize()
    return [t.detach().double().cpu().reshape(-1, *t.shape[-2:]) for t in o]


def _pair(tag, B, hw):
    return seeded(f"{tag}.left", B, 3, *hw).cuda(), seeded(f"{tag}.right", B, 3, *hw).cuda()


def test_cmf_accuracy_256x512(ecm):
    z = _z("g13_full_cmf_256x512_fp64")
    left, right = seeded("g13.left_full", 1, 3, 256, 512).cuda(), seeded("g13.right_full", 1, 3, 256, 512).cuda()
    ref = [torch.from_numpy(z[f"o{i}_64"]).reshape(1, *z[f"o{i}_64"].shape[-2:]) for i in (1, 2, 3)]
    model = _model(ecm, "cmf")
    f32 = _run(ecm, model, left, right, "fp32")
    for mode in ("dec", "all"):
        emu = _run(ecm, model, left, right, mode + "_emu")
        b16 = _run(ecm, model, left, right, mode)
        for i, (r, e, b, f) in enumerate(zip(ref, emu, b16, f32)):
            assert b.shape == f.shape and not torch.equal(b, f), (mode, i)          # the bf16 path was taken
            _bar(f"cmf (256, 512) {mode:3s} head {i + 1}", r, e[..., ::4, ::4], b[..., ::4, ::4])


def test_decoder_result_is_fp32_per_head(ecm):
    model = _model(ecm, "cmf")
    left, right = _pair("dt", 2, (256, 512))
    with torch.no_grad(), ecm.ops.decoder_dtype(BF):
        o = model(left, right)
    assert len(o) == 3 and all(t.dtype == torch.float32 and tuple(t.shape) == (2, 1, 256, 512) for t in o)


def test_fp32_and_the_other_switches_unaffected(ecm):
    """fp32 is bit-identical before and after `dec` and `all` blocks (with and without frozen_weights()); `enc` and `agg` alone
    give the same bits before and after a `dec` block; two `all` forwards are bit-identical."""
    model = _model(ecm, "cmf")
    left, right = _pair("fp", 1, (256, 512))
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    for ctx in (contextlib.nullcontext, ecm.ops.frozen_weights):
        with ctx():
            a = _run(ecm, model, left, right, "fp32")
            enc, agg = _run(ecm, model, left, right, "enc"), _run(ecm, model, left, right, "agg")
            d = _run(ecm, model, left, right, "dec")
            al = _run(ecm, model, left, right, "all")
            assert same(a, _run(ecm, model, left, right, "fp32")), ctx
            assert same(enc, _run(ecm, model, left, right, "enc")) and same(agg, _run(ecm, model, left, right, "agg")), ctx
            assert same(al, _run(ecm, model, left, right, "all")) and same(d, _run(ecm, model, left, right, "dec")), ctx
        assert not same(a, d) and not same(d, al)


def test_frozen_weights_caches_bf16_deconv_image(ecm):
    model = _model(ecm, "cmf")
    left, right = _pair("fw", 1, (256, 512))
    plain = _run(ecm, model, left, right, "dec")
    with ecm.ops.frozen_weights():
        a = _run(ecm, model, left, right, "dec")
        w = model.srr.deconv_module_list[1][0].weight
        assert "bf16_deconv2d" in w._ecm_packed and "bf16_conv2d" in model.srr.conv2[0][0].weight._ecm_packed
        cached = w._ecm_packed["bf16_deconv2d"][1]
        b = _run(ecm, model, left, right, "dec")
        assert w._ecm_packed["bf16_deconv2d"][1] is cached
        ecm.ops.invalidate_packed()
        c = _run(ecm, model, left, right, "dec")
        assert w._ecm_packed["bf16_deconv2d"][1] is not cached
    assert all(torch.equal(x, y) and torch.equal(x, u) and torch.equal(x, v) for x, y, u, v in zip(plain, a, b, c))
    assert all(k.dtype == torch.float32 for k in model.state_dict().values())


def test_grad_enabled_forward_raises_before_any_launch(ecm):
    model = _model(ecm, "cmf")
    left, right = _pair("gr", 1, (256, 512))
    before = _run(ecm, model, left, right, "fp32")
    calls = []
    real_call = ecm._lib.call

    def rec(name, *args):
        calls.append(name)
        return real_call(name, *args)
    ecm._lib.call = rec
    try:
        with ecm.ops.decoder_dtype(BF), pytest.raises(RuntimeError, match="no backward"):
            model(left, right)
    finally:
        ecm._lib.call = real_call
    assert calls == [], calls
    assert all(torch.equal(x, y) for x, y in zip(before, _run(ecm, model, left, right, "fp32")))


@pytest.mark.parametrize("arch", [a for a in ARCHS if a != "cmf"])
def test_architectures_without_a_decoder_are_unchanged(ecm, arch):
    model = _model(ecm, arch)
    left, right = _pair("nd", 1, (256, 512))
    a = _run(ecm, model, left, right, "fp32")
    b = _run(ecm, model, left, right, "dec")
    assert all(torch.equal(x, y) for x, y in zip(a, b)), arch


def test_h_or_w_not_a_multiple_of_4_raises_as_in_fp32(ecm):
    model = _model(ecm, "cmf")
    x = torch.zeros(1, 3, 258, 512, device="cuda")
    with torch.no_grad(), ecm.ops.decoder_dtype(BF), pytest.raises(ValueError, match="multiples of 4"):
        model(x, x)


@pytest.mark.parametrize("hw", [(576, 960), (384, 1248)])
def test_no_slow_path_bf16_decoder(ecm, hw):
    model = _model(ecm, "cmf")
    left, right = _pair("sp", 1, hw)
    for mode in ("dec", "all"):
        ecm.models.SLOW_PATH_EVENTS.clear()
        o = _run(ecm, model, left, right, mode)
        assert ecm.models.SLOW_PATH_EVENTS == [], (mode, ecm.models.SLOW_PATH_EVENTS)
        assert all(tuple(t.shape[-2:]) == hw and bool(torch.isfinite(t).all()) for t in o), mode


def test_no_aten_convolution_or_group_norm_in_the_region(ecm):
    """The region's launches: only the library's entry points compute (ATen contributes casts, views and concatenations)."""
    from torch.profiler import ProfilerActivity, profile
    srr = ecm.super_resolution_refinement(32, 2).cuda().eval()
    ins = (_R(3, 1, 8, 16).abs(), _R(1, 3, 32, 64), _R(1, 32, 8, 16), _R(1, 32, 16, 32))
    with torch.no_grad(), ecm.ops.decoder_dtype(BF), profile(activities=[ProfilerActivity.CPU]) as prof:
        srr(*ins)
    names = {e.key for e in prof.key_averages()}
    assert any(n.startswith("aten::") for n in names), sorted(names)           # ATen's operators are what the profile names
    bad = [n for n in names if n.startswith("aten::") and any(k in n.lower() for k in ("conv", "group_norm", "batch_norm", "miopen"))]
    assert not bad, bad                                                         # (the library's own autograd Functions aside)


def test_decoder_bf16_eval_faster_b4_576x960(ecm):
    model = _model(ecm, "cmf")
    left, right = _pair("tm", 4, (576, 960))

    def ms(dec):
        with torch.no_grad(), ecm.ops.frozen_weights(), ecm.ops.aggregation_dtype(BF), ecm.ops.encoder_dtype(BF), \
                (ecm.ops.decoder_dtype(BF) if dec else contextlib.nullcontext()):
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
    two, three = ms(False), ms(True)
    print(f"cmf eval B=4 576x960: encoder + aggregation bf16 {two:.2f} ms, all three bf16 {three:.2f} ms, ratio {two / three:.2f}")
    assert three < two, (two, three)
