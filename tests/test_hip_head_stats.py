"""Per-pixel uncertainty of the disparity heads on the MI355X: ops.ecm_aggregate9_stats,
ops.volume_mapping_stats, ops.trilinear_softargmin_stats and _ECMNet.predict.

Reference and yardstick.  q64 = the torch restatement of tests/test_head_stats_cpu.py (eight_t, volume_t,
trilinear_t3) in fp64 on the CPU; e32(q) = the distance from q64 of the same restatement in fp32 on the device (softmax, then
the centred moments), per case.  A kernel passes when  max|q - q64| <= 4 * e32(q) + 2e-7 * max|q64|  over every element of the
case, for q in std, peak, entropy.  Each check prints `HSRATIO <path> <quantity> <ratio>`, ratio = error / bound; DESIGN.md
section 15 records the worst per path.

Shapes are the smallest that reach every branch: eight at 3 x 5 cells (every border and corner, so every pattern of skipped
neighbours) and 1 x 1; volume at Dl = 3, 2 x 3 cells (pixels with X < D take the ones-initialised target weights, j = 0 and
j = Dl - 1 lack a depth neighbour); trilinear to 8 x 12 and to the non-multiple 7 x 11.  The disparity every new entry point
also writes must equal the existing kernels' bit for bit on every case."""
import math

import pytest
import torch

from oracle.weights import seeded
from test_head_stats_cpu import eight_t, one_hot_w9, trilinear_t3, volume_t
from test_hip_context_fp64 import mlp_weights, tri_src
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, FLOOR = 4, 2e-7
QUANT = ("std", "peak", "entropy")


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def yardstick(path, case, got, ref_fn, operands, D):
    """got = (disp, std, peak, entropy) of the kernel; ref_fn(*operands) the restatement.  The bound on std / peak / entropy,
    and the ranges that hold everywhere."""
    q64 = ref_fn(*[t.double().cpu() if torch.is_tensor(t) else t for t in operands])
    q32 = ref_fn(*operands)
    fails = []
    for name, g, r64, r32 in zip(QUANT, got[1:], q64[1:], q32[1:]):
        err = float((g.double().cpu() - r64).abs().max())
        e32, scale = float((r32.double().cpu() - r64).abs().max()), float(r64.abs().max())
        bound = K * e32 + FLOOR * scale
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"HSRATIO {path} {name} {ratio:.3f}   # {case}: err {err:.3e}, e32 {e32:.3e}, max|ref| {scale:.3e}")
        if not err <= bound:
            fails.append(f"{case}: {name} on {path}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")
    _, std, peak, ent = got
    if not bool((std >= 0).all()):
        fails.append(f"{case}: std < 0 or NaN")
    if not bool(((peak > 0) & (peak <= 1)).all()):
        fails.append(f"{case}: peak outside (0, 1]")
    if not bool(((ent >= 0) & (ent <= math.log(D) * (1 + 1e-6))).all()):
        fails.append(f"{case}: entropy outside [0, ln {D}]: {float(ent.min()):.3e} .. {float(ent.max()):.9f}")
    assert not fails, "\n".join(fails)


# ---- eight -----------------------------------------------------------------------------------------------------------------------------
def eight_operands(ecm, NH, B, D, h, w, s, scale, hot):
    n = f"hs.eight.{NH}.{h}x{w}.{scale}"
    c = seeded(n + ".c", NH, B, D, h, w, scale=float(scale)).to(DEV)
    if hot:
        return c, one_hot_w9(B, h * s, w * s, dtype=torch.float32).to(DEV)
    lr, hr = seeded(n + ".lr", B, 32, h, w).to(DEV), seeded(n + ".hr", B, 32, h * s, w * s).to(DEV)
    return c, ecm.ops.ecm_weights9(lr, hr, *[t.to(DEV) for t in mlp_weights()])


@pytest.mark.parametrize("hot", [False, True], ids=["weights9", "onehot"])
@pytest.mark.parametrize("scale", [1, 8, 40])
@pytest.mark.parametrize("NH,h,w", [(1, 3, 5), (3, 3, 5), (3, 1, 1)])
def test_eight_against_fp64(ecm, NH, h, w, scale, hot):
    ops, B, D, s = ecm.ops, 2, 5, 4
    c, w9 = eight_operands(ecm, NH, B, D, h, w, s, scale, hot)
    got = ops.ecm_aggregate9_stats(c, w9, s)
    assert all(t.shape == (NH, B, h * s, w * s) and t.dtype == torch.float32 and not t.requires_grad for t in got)
    assert torch.equal(got[0], ops.ecm_aggregate9(ops.softargmin_heads(c), w9, s))
    yardstick("eight", f"NH{NH} {h}x{w} x{scale} {'onehot' if hot else 'weights9'}", got, eight_t, (c, w9, s), D)
    ops.check_async_errors()


# ---- volume ----------------------------------------------------------------------------------------------------------------------------
def volume_operands(NH, B, Dl, h, w, s):
    n = f"hs.volume.{NH}.{s}"
    return (seeded(n + ".c", NH, B, Dl, h, w, scale=1.5).to(DEV), seeded(n + ".m5", B, 5, h * s, w * s, scale=0.5).to(DEV),
            seeded(n + ".mt3", B, 3, h * s, w * s, scale=0.5).to(DEV))


@pytest.mark.parametrize("NH", [1, 3])
@pytest.mark.parametrize("s", [4, 16])
def test_volume_against_fp64(ecm, NH, s):
    ops, B, Dl, h, w = ecm.ops, 2, 3, 2, 3
    c, m5, mt3 = volume_operands(NH, B, Dl, h, w, s)
    assert Dl * s > 1 and w * s > 1                                  # pixels with X < D exist (the ones-initialised branch)
    got = ops.volume_mapping_stats(c, m5, mt3, s)
    assert all(t.shape == (NH, B, h * s, w * s) and not t.requires_grad for t in got)
    assert torch.equal(got[0], ops.volume_mapping(c, m5, mt3, s))
    yardstick("volume", f"NH{NH} s{s}", got, volume_t, (c, m5, mt3, s), Dl * s)
    ops.check_async_errors()


# ---- trilinear -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NH", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 12), (7, 11)])
def test_trilinear_against_fp64(ecm, NH, H, W):
    ops, B, Dl, h, w, Do = ecm.ops, 2, 3, 2, 3, 12
    c = seeded(f"hs.tri.{NH}", NH, B, Dl, h, w, scale=1.5).to(DEV)
    got = ops.trilinear_softargmin_stats(c, Do, H, W)
    assert all(t.shape == (NH, B, H, W) and not t.requires_grad for t in got)
    assert torch.equal(got[0], ops.trilinear_softargmin(c, Do, H, W))
    yardstick("trilinear", f"NH{NH} {H}x{W}", got, trilinear_t3, (c, Do, H, W), Do)
    ops.check_async_errors()


# ---- closed forms on the device ---------------------------------------------------------------------------------------------------------
# Tolerance: at most 28 terms, each within two fp32 roundings (2.4e-7) of its share: 1e-5 of max(1, |value|).
def close(t, value):
    return bool(((t - value).abs() <= 1e-5 * max(1.0, abs(value))).all())


def spike_logits(NH, B, D, h, w, at):
    c = torch.zeros(NH, B, D, h, w, device=DEV)
    for d in at:
        c[0, :, d] = 60.0                                            # in c_0: every head's cumulative logits carry it
    return c


def test_closed_forms_eight(ecm):
    ops, B, D, h, w, s = ecm.ops, 2, 5, 3, 5, 4
    w9 = eight_operands(ecm, 3, B, D, h, w, s, 1, False)[1]
    for w9_ in (w9, one_hot_w9(B, h * s, w * s, dtype=torch.float32).to(DEV)):       # every cell alike: any mixture is the cell
        _, std, peak, ent = ops.ecm_aggregate9_stats(torch.zeros(3, B, D, h, w, device=DEV), w9_, s)
        assert close(std, s * math.sqrt((D * D - 1) / 12)) and close(peak, 1 / D) and close(ent, math.log(D))
        _, std, peak, ent = ops.ecm_aggregate9_stats(spike_logits(3, B, D, h, w, (0, 3)), w9_, s)
        assert close(std, s * 1.5) and close(peak, 0.5) and close(ent, math.log(2))
        _, std, peak, ent = ops.ecm_aggregate9_stats(spike_logits(3, B, D, h, w, (2,)), w9_, s)
        assert bool((std < 1e-6).all()) and bool((1 - peak < 1e-6).all()) and bool((ent < 1e-6).all())
    # one-hot on the centre: the cell's own statistics, std times s
    c = eight_operands(ecm, 3, B, D, h, w, s, 8, True)[0]
    got = ops.ecm_aggregate9_stats(c, one_hot_w9(B, h * s, w * s, dtype=torch.float32).to(DEV), s)
    p = torch.softmax(torch.cumsum(c.double(), 0), 2)
    idx = torch.arange(D, device=DEV, dtype=torch.float64).view(1, 1, D, 1, 1)
    mu = (p * idx).sum(2, keepdim=True)
    std_c = (p * (idx - mu) ** 2).sum(2).sqrt()
    up = lambda t: t.repeat_interleave(s, -1).repeat_interleave(s, -2)                # noqa: E731
    assert bool(((got[1] - s * up(std_c)).abs() <= 1e-5 * s * D).all())
    assert bool(((got[2] - up(p.amax(2))).abs() <= 1e-5).all())


def test_closed_forms_volume(ecm):
    """Centre-only m5 and all-ones target planes: v[D] = c[j-1] + c[j] + c[j+1] at every pixel, j = D // s."""
    ops, B, Dl, h, w, s = ecm.ops, 1, 7, 2, 3, 4
    H, W, D = h * s, w * s, Dl * s
    m5 = torch.zeros(B, 5, H, W, device=DEV)
    m5[:, 0] = 1
    mt3 = torch.ones(B, 3, H, W, device=DEV)
    _, std, peak, ent = ops.volume_mapping_stats(torch.zeros(3, B, Dl, h, w, device=DEV), m5, mt3, s)
    assert close(std, math.sqrt((D * D - 1) / 12)) and close(peak, 1 / D) and close(ent, math.log(D))
    # spikes at j = 1 and j = 5: two plateaus of 3 s disparities, [0, 3 s) and [4 s, 7 s), their centres 4 s apart
    _, std, peak, ent = ops.volume_mapping_stats(spike_logits(3, B, Dl, h, w, (1, 5)), m5, mt3, s)
    assert close(std, math.sqrt(((3 * s) ** 2 - 1) / 12 + (2 * s) ** 2)) and close(peak, 1 / (6 * s)) and close(ent, math.log(6 * s))
    # one spike at j = 0 and zero side planes: one plateau of s, on the pixels that read the planes for every D < 2 s (at
    # X < D the ones-initialised side weights bring the spike back in from the neighbouring depth)
    mt3[:, 1:] = 0
    disp, std, peak, ent = ops.volume_mapping_stats(spike_logits(3, B, Dl, h, w, (0,)), m5, mt3, s)
    inside = torch.arange(W, device=DEV).view(1, 1, 1, W).expand_as(std) >= 2 * s - 1
    assert close(std[inside], math.sqrt((s * s - 1) / 12)) and close(peak[inside], 1 / s) and close(ent[inside], math.log(s))


def test_closed_forms_trilinear(ecm):
    """Identity resampling (Do, H, W) = (Dl, h, w): the logits are c itself."""
    ops, B, D, h, w = ecm.ops, 2, 12, 2, 3
    _, std, peak, ent = ops.trilinear_softargmin_stats(torch.full((3, B, D, h, w), 0.25, device=DEV), D, h, w)
    assert close(std, math.sqrt((D * D - 1) / 12)) and close(peak, 1 / D) and close(ent, math.log(D))
    disp, std, peak, ent = ops.trilinear_softargmin_stats(spike_logits(3, B, D, h, w, (2, 9)), D, h, w)
    assert close(disp, 5.5) and close(std, 3.5) and close(peak, 0.5) and close(ent, math.log(2))
    _, std, peak, ent = ops.trilinear_softargmin_stats(spike_logits(3, B, D, h, w, (7,)), D, h, w)
    assert bool((std < 1e-6).all()) and bool((1 - peak < 1e-6).all()) and bool((ent < 1e-6).all())
    # upsampled uniform logits stay uniform
    _, std, peak, ent = ops.trilinear_softargmin_stats(torch.zeros(1, B, 3, h, w, device=DEV), 12, 7, 11)
    assert close(std, math.sqrt(143 / 12)) and close(peak, 1 / 12) and close(ent, math.log(12))


# ---- a NaN logit reaches exactly the pixels that read it ---------------------------------------------------------------------------------
def nan_check(got, want, what):
    for name, t in zip(("disp",) + QUANT, got):
        assert torch.equal(torch.isnan(t), want.expand_as(t)), f"{what}: {name}: NaN pixels are not exactly the readers of the NaN logit"


def test_nan_logit_eight(ecm):
    ops, NH, B, D, h, w, s = ecm.ops, 3, 2, 5, 3, 5, 4
    c, w9 = eight_operands(ecm, NH, B, D, h, w, s, 8, False)
    c[0, 0, 2, 1, 2] = float("nan")                                  # cell (1,2) of sample 0: its 3 x 3 neighbourhood reads it
    want = torch.zeros(1, B, h * s, w * s, dtype=torch.bool, device=DEV)
    want[0, 0, 0:3 * s, 1 * s:4 * s] = True
    nan_check(ops.ecm_aggregate9_stats(c, w9, s), want, "eight")
    c2, _ = eight_operands(ecm, NH, B, D, h, w, s, 8, False)
    c2[0, 1, 0, 0, 0] = float("nan")                                 # a corner cell: the neighbours outside are not read
    want = torch.zeros(1, B, h * s, w * s, dtype=torch.bool, device=DEV)
    want[0, 1, 0:2 * s, 0:2 * s] = True
    nan_check(ops.ecm_aggregate9_stats(c2, w9, s), want, "eight corner")


def test_nan_logit_volume(ecm):
    ops, NH, B, Dl, h, w, s = ecm.ops, 3, 2, 3, 2, 3, 4
    c, m5, mt3 = volume_operands(NH, B, Dl, h, w, s)
    c[0, 0, 1, 0, 1] = float("nan")                                  # cell (0,1): itself and its l, r, b neighbours fuse it
    cells = torch.zeros(h, w, dtype=torch.bool)
    for y, x in ((0, 1), (0, 0), (0, 2), (1, 1)):
        cells[y, x] = True
    want = torch.zeros(1, B, h * s, w * s, dtype=torch.bool, device=DEV)
    want[0, 0] = cells.repeat_interleave(s, 0).repeat_interleave(s, 1).to(DEV)
    nan_check(ops.volume_mapping_stats(c, m5, mt3, s), want, "volume")


def test_nan_logit_trilinear(ecm):
    ops, NH, B, Dl, h, w, Do, H, W = ecm.ops, 3, 2, 3, 2, 3, 12, 7, 11
    c = seeded("hs.tri.nan", NH, B, Dl, h, w, scale=1.5).to(DEV)
    c[0, 1, 1, 0, 1] = float("nan")                                  # plane 1 (every pixel's sweep samples it), cell (0,1)
    assert any(1 in tri_src(D, Dl / Do, Dl) for D in range(Do))
    want = torch.zeros(1, B, H, W, dtype=torch.bool, device=DEV)
    for Y in range(H):
        for X in range(W):
            want[0, 1, Y, X] = 0 in tri_src(Y, h / H, h) and 1 in tri_src(X, w / W, w)
    nan_check(ops.trilinear_softargmin_stats(c, Do, H, W), want, "trilinear")


# ---- guard bands around stats, lse and disp ----------------------------------------------------------------------------------------------
def test_guard_bands(ecm):
    ops = ecm.ops
    c, w9 = eight_operands(ecm, 3, 2, 5, 3, 5, 4, 8, False)
    with guarded(ecm) as g:
        ops.ecm_aggregate9_stats(c, w9, 4)
        g.check("ecm_aggregate9_stats")
        assert len(g.records) == 4                                   # d, lse, disp, stats
    with guarded(ecm) as g:
        ops.volume_mapping_stats(*volume_operands(3, 2, 3, 2, 3, 4), 4)
        g.check("volume_mapping_stats")
    with guarded(ecm) as g:
        ops.trilinear_softargmin_stats(seeded("hs.tri.3", 3, 2, 3, 2, 3, scale=1.5).to(DEV), 12, 7, 11)
        g.check("trilinear_softargmin_stats")


def test_refusals_match_the_parents(ecm):
    ops = ecm.ops
    c = torch.zeros(4, 1, 3, 2, 3, device=DEV)                       # four heads: ECM_EUNSUP, as the plain heads
    with pytest.raises(RuntimeError):
        ops.trilinear_softargmin_stats(c, 12, 8, 12)
    with pytest.raises(RuntimeError):
        ops.volume_mapping_stats(c, torch.zeros(1, 5, 8, 12, device=DEV), torch.zeros(1, 3, 8, 12, device=DEV), 4)
    with pytest.raises(RuntimeError):
        ops.ecm_aggregate9_stats(torch.zeros(4, 1, 3, 2, 3, device=DEV), torch.zeros(1, 9, 8, 12, device=DEV), 4)
    with pytest.raises(RuntimeError, match="w9"):
        ops.ecm_aggregate9_stats(c[:3], torch.zeros(1, 9, 8, 11, device=DEV), 4)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.trilinear_softargmin_stats(c[:3].cpu(), 12, 8, 12)
    ops.check_async_errors()


# ---- predict ---------------------------------------------------------------------------------------------------------------------------
STATS_OP = {"eight": "ecm_aggregate9_stats", "volume": "volume_mapping_stats", "trilinear": "trilinear_softargmin_stats"}


def _frames(H, W, B=1):
    g = torch.Generator(device=DEV).manual_seed(11)
    return torch.randn(B, 3, H, W, device=DEV, generator=g), torch.randn(B, 3, H, W, device=DEV, generator=g)


@pytest.mark.parametrize("arch", ["cmfsm", "cmfsm_sub_16", "cm_sub_8", "bilinear_cmf"])
def test_predict_256x512(ecm, arch):
    """256 x 512 is the smallest frame these nets take: their encoders pool the quarter-resolution map by 64."""
    H, W = 256, 512
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    left, right = _frames(H, W)
    with torch.no_grad():
        fwd = model(left, right)
    pred = model.predict(left, right)
    assert all(len(f) == 3 for f in pred)
    for k in range(3):
        assert all(f[k].shape == (1, 1, H, W) and not f[k].requires_grad for f in pred)
        assert torch.equal(pred.disparity[k], fwd[k].reshape(1, 1, H, W)), f"{arch}: head {k} differs from forward"
        assert bool(torch.isfinite(pred.std[k]).all()) and bool((pred.peak[k] > 0).all()) and bool((pred.entropy[k] >= 0).all())
    last = model.predict(left, right, heads=(2,))
    assert all(len(f) == 1 and torch.equal(f[0], g[2]) for f, g in zip(last, pred))
    # the statistics are the op-level call on the model's own logits
    with torch.no_grad():
        fields, args = model.head_stats(left, right)
    again = getattr(ops, STATS_OP[model.HEAD])(*args)
    NH = args[0].shape[0]
    assert NH == model.HOURGLASSES
    for f, a, b in zip(pred, fields, again):
        assert torch.equal(a, b) and all(torch.equal(f[k][:, 0], a[min(k, NH - 1)]) for k in range(3))
    with ops.inference_dtype(torch.bfloat16), ops.frozen_weights(), torch.no_grad():
        fwd16 = model(left, right)
        pred16 = model.predict(left, right)
    for k in range(3):
        assert torch.equal(pred16.disparity[k], fwd16[k].reshape(1, 1, H, W)), f"{arch}: bf16 head {k} differs from forward"
        assert bool(torch.isfinite(pred16.std[k]).all())
    ops.check_async_errors()


def test_predict_full_frame_cmfsm(ecm):
    """A size check of the index arithmetic at 576 x 960 (553 k pixels x 9 columns of 48), not an accuracy check."""
    torch.manual_seed(5)
    model = ecm.get_model("cmfsm").to(DEV).eval()
    left, right = _frames(576, 960)
    with ecm.ops.frozen_weights():
        pred = model.predict(left, right)
    for f in pred:
        assert len(f) == 3 and all(t.shape == (1, 1, 576, 960) and bool(torch.isfinite(t).all()) for t in f)
    assert all(bool((t >= 0).all()) for t in pred.std) and all(bool(((t > 0) & (t <= 1)).all()) for t in pred.peak)
    assert all(bool(((t >= 0) & (t <= math.log(48) * (1 + 1e-6))).all()) for t in pred.entropy)
    ecm.ops.check_async_errors()
