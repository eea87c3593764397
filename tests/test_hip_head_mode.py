"""The modal disparity of the heads on the MI355X: ops.ecm_aggregate9_mode, ops.volume_mapping_mode,
ops.trilinear_softargmin_mode and predict(mode_radius=...).

Reference and yardstick (sections 14 and 15).  p64 = the distribution of the head restated in fp64 on the CPU
(tests/test_head_mode_cpu.py: eight_p, volume_p, trilinear_p), p32 the same restatement in fp32 on the device.  Both sides are
evaluated by modal_t with the window about the KERNEL'S OWN index, so mode and mass are smooth in the inputs and the argmax
question is separate:  max|q - q64| <= 4 e32(q) + 2e-7 max|q64|  over every element of the case, q in mode, mass.  The argmax:
index is an integer multiple of u inside the range; p64[index] >= max p64 (1 - tol), tol = 4 e32rel(p) + 2e-7 with e32rel the
largest relative error of p32; and at most 1 % of a case's pixels may have an index other than the fp64 argmax (levels that
fp64 itself cannot tell apart, TIE64 below, count as that argmax).  Each check
prints `HMRATIO <path> <quantity> <ratio>`, ratio = error / bound; section 16 records the worst per path.

Shapes, eight (s = 4 unless said): 3 x 5 cells with D' = 12 (every border and corner), 1 x 1 with D' = 6 (eight invalid
neighbours), 2 x 3 with D' = 48 (the full-size column, one chunk), 3 x 19 with D' = 5 (the kernel's tile is 64 x 4 pixels =
16 x 1 cells, 18 x 3 staged: one cell wider and one taller, so two tiles along X and three along Y with a ragged last tile),
2 x 3 with D' = 7 (no multiple of anything) and, beyond the issue's list, 2 x 3 with D' = 55 (two chunks of levels, 48 + 7:
the re-staging path) and 3 x 5 at s = 2 (a tile spanning two cell rows).  Volume: Dl = 3 at s = 4 and 16; trilinear to
8 x 12 and 7 x 11."""
import ctypes as C

import pytest
import torch

from oracle.weights import seeded
from test_head_mode_cpu import eight_p, modal_t, trilinear_p, volume_p
from test_head_stats_cpu import one_hot_w9, valid9
from test_hip_context_fp64 import tri_src
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, FLOOR, SHARE = 4, 2e-7, 0.01
# Two levels of p64 closer than this are ONE maximum for the fp64 restatement too, and an index on either is its argmax: the
# trilinear head's top levels (those whose source depth is clamped to the last plane: D = 10, 11 of 12 from Dl = 3) are equal in
# exact arithmetic and differ in fp64 only by the rounding of w0 * a + w1 * a, ~1e-16; 1e-12 is ten thousand such roundings.
TIE64 = 1e-12


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


class Ref:
    """The distribution of one case, restated once: p64 on the CPU, p32 on the device, and what the argmax conditions need."""

    def __init__(self, p_fn, operands, u):
        self.u = u
        self.p64 = p_fn(*[t.double().cpu() if torch.is_tensor(t) else t for t in operands])
        self.p32 = p_fn(*operands)
        self.L = self.p64.shape[2]
        rel = ((self.p32.double().cpu() - self.p64).abs() / self.p64)
        self.tol = K * float(rel[self.p64 > 0].max()) + FLOOR
        self.top, self.arg = self.p64.max(2)


def yardstick(path, case, got, ref, radius):
    """got = (mode, mass, index) of the kernel at `radius` full-resolution pixels."""
    mode, mass, index = (t.double().cpu() for t in got)
    u, L, fails = ref.u, ref.L, []
    lev = torch.round(index / u)
    if not (bool((lev * u == index).all()) and bool(((lev >= 0) & (lev < L)).all())):
        raise AssertionError(f"{case}: index on {path} is not an integer multiple of {u} inside [0, {u * L})")
    lev = lev.long()
    at = ref.p64.gather(2, lev.unsqueeze(2)).squeeze(2)
    if not bool((at >= ref.top * (1 - ref.tol)).all()):
        fails.append(f"{case}: index on {path}: p64[index] < max p64 * (1 - {ref.tol:.2e}); worst ratio {float((at / ref.top).min()):.9f}")
    share = float(((lev != ref.arg) & (at < ref.top * (1 - TIE64))).double().mean())
    print(f"HMSHARE {path} {share:.5f}   # {case} r{radius}: pixels whose index is not the fp64 argmax")
    if not share <= SHARE:
        fails.append(f"{case}: index on {path}: {share:.3%} of the pixels differ from the fp64 argmax (cap {SHARE:.0%})")
    _, mode64, mass64 = modal_t(ref.p64, radius // u, index=lev)
    _, mode32, mass32 = modal_t(ref.p32, radius // u, index=lev.to(ref.p32.device))
    for name, g, r64, r32 in (("mode", mode, u * mode64, u * mode32), ("mass", mass, mass64, mass32)):
        err = float((g - r64).abs().max())
        e32, scale = float((r32.double().cpu() - r64).abs().max()), float(r64.abs().max())
        bound = K * e32 + FLOOR * scale
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"HMRATIO {path} {name} {ratio:.3f}   # {case} r{radius}: err {err:.3e}, e32 {e32:.3e}, max|ref| {scale:.3e}")
        if not err <= bound:
            fails.append(f"{case} r{radius}: {name} on {path}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")
    if not bool(((got[1] > 0) & (got[1] <= 1)).all()):
        fails.append(f"{case} r{radius}: mass outside (0, 1]")
    if not bool(((got[0] - got[2]).abs() <= radius).all()):
        fails.append(f"{case} r{radius}: mode further than the radius from index")
    assert not fails, "\n".join(fails)


# ---- eight -----------------------------------------------------------------------------------------------------------------------------
EIGHT_SHAPES = [(3, 5, 12, 4), (1, 1, 6, 4), (2, 3, 48, 4), (3, 19, 5, 4), (2, 3, 7, 4), (2, 3, 55, 4), (3, 5, 12, 2)]


def eight_operands(NH, B, D, h, w, s, scale, hot):
    n = f"hm.eight.{NH}.{h}x{w}.{D}.{s}.{scale}"
    c = seeded(n + ".c", NH, B, D, h, w, scale=float(scale)).to(DEV)
    if hot:
        return c, one_hot_w9(B, h * s, w * s, dtype=torch.float32).to(DEV)
    return c, torch.softmax(seeded(n + ".w9", B, 9, h * s, w * s), 1).to(DEV)


@pytest.mark.parametrize("hot", [False, True], ids=["softmax9", "onehot"])
@pytest.mark.parametrize("scale", [1, 8, 40])
@pytest.mark.parametrize("h,w,D,s", EIGHT_SHAPES)
def test_eight_against_fp64(ecm, h, w, D, s, scale, hot):
    ops, NH, B = ecm.ops, 3, 2
    c, w9 = eight_operands(NH, B, D, h, w, s, scale, hot)
    ref = Ref(eight_p, (c, w9, s), s)
    for radius in (0, s, 2 * s, s * (D - 1)):
        got = ops.ecm_aggregate9_mode(c, w9, s, radius)
        assert all(t.shape == (NH, B, h * s, w * s) and t.dtype == torch.float32 and not t.requires_grad for t in got)
        yardstick("eight", f"{h}x{w} D{D} s{s} x{scale} {'onehot' if hot else 'softmax9'}", got, ref, radius)
    ops.check_async_errors()


# ---- volume ----------------------------------------------------------------------------------------------------------------------------
def volume_operands(NH, B, Dl, h, w, s):
    n = f"hm.volume.{NH}.{s}"
    return (seeded(n + ".c", NH, B, Dl, h, w, scale=1.5).to(DEV), seeded(n + ".m5", B, 5, h * s, w * s, scale=0.5).to(DEV),
            seeded(n + ".mt3", B, 3, h * s, w * s, scale=0.5).to(DEV))


@pytest.mark.parametrize("NH", [1, 3])
@pytest.mark.parametrize("s", [4, 16])
def test_volume_against_fp64(ecm, NH, s):
    ops, B, Dl, h, w = ecm.ops, 2, 3, 2, 3
    c, m5, mt3 = volume_operands(NH, B, Dl, h, w, s)
    ref = Ref(volume_p, (c, m5, mt3, s), 1)
    for radius in (0, 1, 4, Dl * s - 1):
        got = ops.volume_mapping_mode(c, m5, mt3, s, radius)
        assert all(t.shape == (NH, B, h * s, w * s) and not t.requires_grad for t in got)
        yardstick("volume", f"NH{NH} s{s}", got, ref, radius)
    ops.check_async_errors()


# ---- trilinear -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NH", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 12), (7, 11)])
def test_trilinear_against_fp64(ecm, NH, H, W):
    ops, B, Dl, h, w, Do = ecm.ops, 2, 3, 2, 3, 12
    c = seeded(f"hm.tri.{NH}", NH, B, Dl, h, w, scale=1.5).to(DEV)
    ref = Ref(trilinear_p, (c, Do, H, W), 1)
    for radius in (0, 1, 4, Do - 1):
        got = ops.trilinear_softargmin_mode(c, Do, H, W, radius)
        assert all(t.shape == (NH, B, H, W) and not t.requires_grad for t in got)
        yardstick("trilinear", f"NH{NH} {H}x{W}", got, ref, radius)
    ops.check_async_errors()


# ---- an exact tie: the lowest index, on the device ---------------------------------------------------------------------------------------
def test_exact_tie_gives_the_lowest_index(ecm):
    """Constant logits: p is uniform, index = 0, mass = (r + 1) / L and mode = u r / 2, each to the yardstick."""
    ops, NH, B = ecm.ops, 3, 2
    for h, w, D, s in ((3, 5, 12, 4), (2, 3, 55, 4)):
        c, w9 = torch.full((NH, B, D, h, w), 0.25, device=DEV), one_hot_w9(B, h * s, w * s, dtype=torch.float32).to(DEV)
        ref = Ref(eight_p, (c, w9, s), s)
        for radius in (0, s, 2 * s, s * (D - 1)):
            got = ops.ecm_aggregate9_mode(c, w9, s, radius)
            assert bool((got[2] == 0).all())
            yardstick("eight", f"tie {h}x{w} D{D}", got, ref, radius)
            r = radius // s
            assert torch.allclose(got[1], torch.full_like(got[1], (r + 1) / D), rtol=1e-5) and torch.allclose(got[0], torch.full_like(got[0], s * r / 2), rtol=1e-5, atol=1e-6)
    Dl, h, w, s = 3, 2, 3, 4
    m5 = torch.zeros(B, 5, h * s, w * s, device=DEV)
    m5[:, 0] = 1
    c, mt3 = torch.zeros(NH, B, Dl, h, w, device=DEV), torch.ones(B, 3, h * s, w * s, device=DEV)      # v[D] = 0 everywhere
    ref = Ref(volume_p, (c, m5, mt3, s), 1)
    for radius in (0, 1, 4, Dl * s - 1):
        got = ops.volume_mapping_mode(c, m5, mt3, s, radius)
        assert bool((got[2] == 0).all())
        yardstick("volume", "tie", got, ref, radius)
    c = torch.full((NH, B, 3, 2, 3), 0.25, device=DEV)
    ref = Ref(trilinear_p, (c, 12, 7, 11), 1)
    for radius in (0, 1, 4, 11):
        got = ops.trilinear_softargmin_mode(c, 12, 7, 11, radius)
        assert bool((got[2] == 0).all())
        yardstick("trilinear", "tie", got, ref, radius)


# ---- the device identities against the statistics ops -------------------------------------------------------------------------------------
def _within_two_bounds(name, a, b, q64, q32):
    """a and b are two device results for the same quantity: each lies within the yardstick's bound of q64, so they lie within
    twice that bound of each other."""
    e32, scale = float((q32.double().cpu() - q64).abs().max()), float(q64.abs().max())
    bound = 2 * (K * e32 + FLOOR * scale)
    err = float((a.double() - b.double()).abs().max())
    assert err <= bound, f"{name}: {err:.3e} > 2 * ({K} * {e32:.3e} + {FLOOR} * {scale:.3e})"


def _identities(name, ref, mode_op, stats, wsum=None):
    u, L = ref.u, ref.L
    disp, _, peak, _ = stats
    mode0, mass0, index0 = mode_op(0)
    assert torch.equal(mode0, index0), f"{name}: radius 0: mode != index"
    _within_two_bounds(name + " mass(0) vs peak", mass0, peak, ref.p64.amax(2), ref.p32.amax(2))
    modeF, massF, _ = mode_op(u * (L - 1))
    idx = torch.arange(L, dtype=torch.float64).view(1, 1, L, 1, 1)
    mu64, mu32 = u * (ref.p64 * idx).sum(2), u * (ref.p32 * idx.float().to(DEV)).sum(2)
    if wsum is not None:                                             # the head's output carries the border factor, the mode does not
        modeF, mu64, mu32 = modeF * wsum, mu64 * wsum.double().cpu(), mu32 * wsum
    _within_two_bounds(name + " mode(full) vs disp", modeF, disp, mu64, mu32)
    _within_two_bounds(name + " mass(full) vs 1", massF, torch.ones_like(massF), ref.p64.sum(2), ref.p32.sum(2))
    assert bool((massF <= 1).all())


def test_radius_zero_and_full_range_against_the_stats_ops(ecm):
    ops, NH, B = ecm.ops, 3, 2
    h, w, D, s = 3, 5, 12, 4
    c, w9 = eight_operands(NH, B, D, h, w, s, 8, False)
    wsum = (w9 * valid9(h, w, s, DEV).to(w9.dtype)).sum(1).unsqueeze(0)
    _identities("eight", Ref(eight_p, (c, w9, s), s), lambda r: ops.ecm_aggregate9_mode(c, w9, s, r), ops.ecm_aggregate9_stats(c, w9, s), wsum)
    c, m5, mt3 = volume_operands(NH, B, 3, 2, 3, 4)
    _identities("volume", Ref(volume_p, (c, m5, mt3, 4), 1), lambda r: ops.volume_mapping_mode(c, m5, mt3, 4, r), ops.volume_mapping_stats(c, m5, mt3, 4))
    c = seeded("hm.tri.3", NH, B, 3, 2, 3, scale=1.5).to(DEV)
    _identities("trilinear", Ref(trilinear_p, (c, 12, 7, 11), 1), lambda r: ops.trilinear_softargmin_mode(c, 12, 7, 11, r), ops.trilinear_softargmin_stats(c, 12, 7, 11))


# ---- a NaN logit reaches exactly the pixels whose support contains it ----------------------------------------------------------------------
def nan_check(got, want, what):
    for name, t in zip(("mode", "mass", "index"), got):
        assert torch.equal(torch.isnan(t), want.expand_as(t)), f"{what}: {name}: NaN pixels are not exactly the readers of the NaN logit"


def test_nan_logit_eight(ecm):
    ops, NH, B, D, h, w, s = ecm.ops, 3, 2, 12, 3, 5, 4
    c, w9 = eight_operands(NH, B, D, h, w, s, 8, False)
    c[0, 0, 2, 1, 2] = float("nan")                                  # cell (1,2) of sample 0: its 3 x 3 neighbourhood reads it
    want = torch.zeros(1, B, h * s, w * s, dtype=torch.bool, device=DEV)
    want[0, 0, 0:3 * s, 1 * s:4 * s] = True
    nan_check(ops.ecm_aggregate9_mode(c, w9, s, s), want, "eight")
    c2, _ = eight_operands(NH, B, D, h, w, s, 8, False)
    c2[0, 1, 0, 0, 0] = float("nan")                                 # a corner cell: the neighbours outside are not read
    want = torch.zeros(1, B, h * s, w * s, dtype=torch.bool, device=DEV)
    want[0, 1, 0:2 * s, 0:2 * s] = True
    nan_check(ops.ecm_aggregate9_mode(c2, w9, s, s), want, "eight corner")
    c3, w93 = eight_operands(NH, B, 55, 2, 3, s, 8, False)           # two chunks of levels: the NaN sits in the second
    c3[0, 0, 50, 0, 0] = float("nan")
    want = torch.zeros(1, B, 2 * s, 3 * s, dtype=torch.bool, device=DEV)
    want[0, 0, :, 0:2 * s] = True
    nan_check(ops.ecm_aggregate9_mode(c3, w93, s, s), want, "eight chunked")


def test_nan_logit_volume(ecm):
    ops, NH, B, Dl, h, w, s = ecm.ops, 3, 2, 3, 2, 3, 4
    c, m5, mt3 = volume_operands(NH, B, Dl, h, w, s)
    c[0, 0, 1, 0, 1] = float("nan")                                  # cell (0,1): itself and its l, r, b neighbours fuse it
    cells = torch.zeros(h, w, dtype=torch.bool)
    for y, x in ((0, 1), (0, 0), (0, 2), (1, 1)):
        cells[y, x] = True
    want = torch.zeros(1, B, h * s, w * s, dtype=torch.bool, device=DEV)
    want[0, 0] = cells.repeat_interleave(s, 0).repeat_interleave(s, 1).to(DEV)
    nan_check(ops.volume_mapping_mode(c, m5, mt3, s, 4), want, "volume")


def test_nan_logit_trilinear(ecm):
    ops, NH, B, Dl, h, w, Do, H, W = ecm.ops, 3, 2, 3, 2, 3, 12, 7, 11
    c = seeded("hm.tri.nan", NH, B, Dl, h, w, scale=1.5).to(DEV)
    c[0, 1, 1, 0, 1] = float("nan")                                  # plane 1 (every pixel's sweep samples it), cell (0,1)
    want = torch.zeros(1, B, H, W, dtype=torch.bool, device=DEV)
    for Y in range(H):
        for X in range(W):
            want[0, 1, Y, X] = 0 in tri_src(Y, h / H, h) and 1 in tri_src(X, w / W, w)
    nan_check(ops.trilinear_softargmin_mode(c, Do, H, W, 4), want, "trilinear")


# ---- guard bands around modal (and the eight head's d and lse) -----------------------------------------------------------------------------
def test_guard_bands(ecm):
    ops = ecm.ops
    for h, w, D, s in EIGHT_SHAPES:
        c, w9 = eight_operands(3, 2, D, h, w, s, 8, False)
        with guarded(ecm) as g:
            ops.ecm_aggregate9_mode(c, w9, s, s)
            g.check(f"ecm_aggregate9_mode {h}x{w} D{D} s{s}")
            assert len(g.records) == 3                               # d, lse, modal
    with guarded(ecm) as g:
        ops.volume_mapping_mode(*volume_operands(3, 2, 3, 2, 3, 4), 4, 4)
        g.check("volume_mapping_mode")
        assert len(g.records) == 1
    with guarded(ecm) as g:
        ops.trilinear_softargmin_mode(seeded("hm.tri.3", 3, 2, 3, 2, 3, scale=1.5).to(DEV), 12, 7, 11, 4)
        g.check("trilinear_softargmin_mode")
        assert len(g.records) == 1


# ---- nheads and the refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NH", [1, 2, 3])
def test_every_head_count(ecm, NH):
    """Head k of an NH-head launch is the cumulative logits c_0 + ... + c_k whatever NH is: the planes of a 3-head launch."""
    ops, B, s = ecm.ops, 2, 4
    c, w9 = eight_operands(3, B, 12, 3, 5, s, 8, False)
    full, part = ops.ecm_aggregate9_mode(c, w9, s, s), ops.ecm_aggregate9_mode(c[:NH], w9, s, s)
    yardstick("eight", f"NH{NH}", part, Ref(eight_p, (c[:NH], w9, s), s), s)
    assert torch.equal(part[2], full[2][:NH])
    cv, m5, mt3 = volume_operands(3, B, 3, 2, 3, s)
    yardstick("volume", f"NH{NH}", ops.volume_mapping_mode(cv[:NH], m5, mt3, s, 4), Ref(volume_p, (cv[:NH], m5, mt3, s), 1), 4)
    ct = seeded("hm.tri.3", 3, B, 3, 2, 3, scale=1.5).to(DEV)
    yardstick("trilinear", f"NH{NH}", ops.trilinear_softargmin_mode(ct[:NH], 12, 7, 11, 4), Ref(trilinear_p, (ct[:NH], 12, 7, 11), 1), 4)


def test_refusals(ecm):
    ops, lib = ecm.ops, ecm._lib.load()
    c = torch.zeros(4, 1, 3, 2, 3, device=DEV)                       # four heads: ECM_EUNSUP, as the plain heads
    with pytest.raises(RuntimeError):
        ops.trilinear_softargmin_mode(c, 12, 8, 12, 4)
    with pytest.raises(RuntimeError):
        ops.volume_mapping_mode(c, torch.zeros(1, 5, 8, 12, device=DEV), torch.zeros(1, 3, 8, 12, device=DEV), 4, 4)
    with pytest.raises(RuntimeError):
        ops.ecm_aggregate9_mode(c, torch.zeros(1, 9, 8, 12, device=DEV), 4, 4)
    ptr = lambda t: C.c_void_p(t.data_ptr())                         # noqa: E731
    lse, w9, modal = torch.zeros(4, 1, 2, 3, device=DEV), torch.zeros(1, 9, 8, 12, device=DEV), torch.zeros(4, 3, 1, 8, 12, device=DEV)
    hs = C.c_longlong(18)
    for nheads in (0, 4):                                            # the C ABI itself: ECM_EUNSUP (-2) outside 1..3
        assert lib.ecm_aggregate9_mode_fwd(ptr(c), hs, ptr(lse), ptr(w9), ptr(modal), nheads, 1, 3, 2, 3, 4, 4, None) == -2
        assert lib.ecm_volume_mapping_mode_fwd(ptr(c), hs, ptr(w9), ptr(w9), ptr(modal), nheads, 1, 3, 2, 3, 4, 4, None) == -2
        assert lib.ecm_trilinear_softargmin_mode_fwd(ptr(c), hs, ptr(modal), nheads, 1, 3, 2, 3, 12, 8, 12, 4, None) == -2
    with pytest.raises(RuntimeError, match="w9"):
        ops.ecm_aggregate9_mode(c[:3], torch.zeros(1, 9, 8, 11, device=DEV), 4, 4)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.trilinear_softargmin_mode(c[:3].cpu(), 12, 8, 12, 4)
    for bad in (-4, 2.0, 6):
        with pytest.raises(ValueError, match="radius"):
            ops.ecm_aggregate9_mode(c[:3], w9, 4, bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="radius"):
            ops.trilinear_softargmin_mode(c[:3], 12, 8, 12, bad)
        with pytest.raises(ValueError, match="radius"):
            ops.volume_mapping_mode(c[:3], torch.zeros(1, 5, 8, 12, device=DEV), torch.zeros(1, 3, 8, 12, device=DEV), 4, bad)
    ops.check_async_errors()


# ---- predict(mode_radius=8) ------------------------------------------------------------------------------------------------------------------
MODE_OP = {"eight": "ecm_aggregate9_mode", "volume": "volume_mapping_mode", "trilinear": "trilinear_softargmin_mode"}


def _frames(H, W, B=1):
    g = torch.Generator(device=DEV).manual_seed(11)
    return torch.randn(B, 3, H, W, device=DEV, generator=g), torch.randn(B, 3, H, W, device=DEV, generator=g)


@pytest.mark.parametrize("arch", ["cmfsm", "cmfsm_sub_16", "bilinear_cmf"])
def test_predict_256x512(ecm, arch):
    """256 x 512, the small input of tests/test_hip_head_stats.py: the first four fields are predict()'s bit for bit."""
    H, W, R = 256, 512, 8
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    left, right = _frames(H, W)
    with torch.no_grad():
        fwd = model(left, right)
    plain, pred = model.predict(left, right), model.predict(left, right, mode_radius=R)
    assert type(plain).__name__ == "Prediction" and len(plain) == 4 and type(pred).__name__ == "ModalPrediction" and len(pred) == 7
    for f, g in zip(plain, pred[:4]):
        assert len(f) == len(g) == 3 and all(torch.equal(a, b) for a, b in zip(f, g))
    L, u = (model.maxdisp // 4, 4) if model.HEAD == "eight" else (model.maxdisp, 1)
    for k in range(3):
        assert torch.equal(pred.disparity[k], fwd[k].reshape(1, 1, H, W)), f"{arch}: head {k} differs from forward"
        assert all(f[k].shape == (1, 1, H, W) and not f[k].requires_grad for f in pred)
        idx = pred.index[k]
        assert bool((idx == torch.round(idx / u) * u).all()) and bool(((idx >= 0) & (idx < L * u)).all())
        assert bool(((pred.mode[k] - idx).abs() <= R).all()) and bool(((pred.mass[k] > 0) & (pred.mass[k] <= 1)).all())
        assert bool((pred.mass[k] >= pred.peak[k] * (1 - 1e-5)).all())                      # the window holds the peak
    last = model.predict(left, right, heads=(2,), mode_radius=R)
    assert all(len(f) == 1 and torch.equal(f[0], g[2]) for f, g in zip(last, pred))
    with torch.no_grad():                                            # the modal planes are the op-level call on the model's own logits
        _, args = model.head_stats(left, right)
    again = getattr(ops, MODE_OP[model.HEAD])(*args, R)
    assert all(torch.equal(f[k][:, 0], a[k]) for f, a in zip(pred[4:], again) for k in range(3))
    with ops.inference_dtype(torch.bfloat16), ops.frozen_weights(), torch.no_grad():
        fwd16 = model(left, right)
        plain16, pred16 = model.predict(left, right), model.predict(left, right, mode_radius=R)
    for f, g in zip(plain16, pred16[:4]):
        assert all(torch.equal(a, b) for a, b in zip(f, g))
    for k in range(3):
        assert torch.equal(pred16.disparity[k], fwd16[k].reshape(1, 1, H, W)), f"{arch}: bf16 head {k} differs from forward"
        assert bool(torch.isfinite(pred16.mode[k]).all()) and bool(((pred16.mode[k] - pred16.index[k]).abs() <= R).all())
    ops.check_async_errors()
