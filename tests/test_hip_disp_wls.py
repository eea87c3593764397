"""The WLS disparity smoother on the MI355X: ops.disparity_wls and _ECMNet.smooth against wls_t, the torch
restatement of tests/test_disp_wls_cpu.py.

Yardstick (sections 14-19): max|hip - out64| <= K e32 + FLOOR max|out64| with K = 4 and FLOOR = 2e-7, for `smoothed` and for
`weight`, out64 = wls_t in fp64 and e32 = the error of wls_t in fp32, both on the device; and the zero patterns are equal.  Worst
ratio measured on the MI355X: 0.591 ([1,65,130], lam 8000), the rest at or below 0.38 (the test prints WLSRATIO lines; DESIGN.md
section 20).

Shapes: the FLOAT_CASES; then with lam = 64, T = 2, C = 1 and 30 % sparse confidences [2,1,1], [1,1,7], [1,7,1], [1,2,3], one
less than / exactly / one more than LINES rows by CHUNK columns (the horizontal pass: LINES rows per workgroup, CHUNK columns per
staged tile), [1, 2 LINES + 1, 2 CHUNK + 1], and the same about VCHUNK rows by VLINES columns for the vertical pass, the constants
read from csrc/disp_wls.hip.  The grid is not capped (a workgroup per LINES lines), so there is no shape for a second round."""
import pytest
import torch

from test_disp_wls_cpu import FLOAT_CASES, FLOAT_IDS, FLOOR, K, KC, float_case, sparse_conf, wls_t
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINES, CHUNK, VLINES, VCHUNK = KC["LINES"], KC["CHUNK"], KC["VLINES"], KC["VCHUNK"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def yardstick(ecm, name, d, g, conf, lam, sc, T):
    """The op against wls_t on the device: asserts the yardstick and the zero patterns, returns (smoothed, weight, weight64)."""
    d, g = d.to(DEV), g.to(DEV)
    conf = None if conf is None else conf.to(DEV)
    got = ecm.ops.disparity_wls(d, g, conf, lam, sc, T, with_weight=True)
    assert all(o.shape == d.shape and o.dtype == torch.float32 for o in got)
    ref32 = wls_t(d, g, conf, lam, sc, T)
    ref64 = wls_t(d.double(), g.double(), None if conf is None else conf.double(), lam, sc, T)
    worst = 0.0
    for what, o, r32, r64 in zip(("smoothed", "weight"), got, ref32, ref64):
        assert bool(torch.isfinite(o).all()), f"{name}: {what} is not finite"
        assert torch.equal(o == 0, r64 == 0), f"{name}: the zero pattern of {what} differs at {int(((o == 0) != (r64 == 0)).sum())} pixels"
        e32 = float((r32.double() - r64).abs().max())
        bound = K * e32 + FLOOR * float(r64.abs().max())
        err = float((o.double() - r64).abs().max())
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else INF)
        print(f"WLSRATIO {name} {what} {ratio:.3f} err {err:.3e} e32 {e32:.3e}")
        worst = max(worst, ratio)
    assert worst <= 1.0, f"{name}: {worst:.3f} of the yardstick"
    return got[0], got[1], ref64[1]


@pytest.mark.parametrize("name,seed,shape,C,lam,sc,T,share", FLOAT_CASES, ids=FLOAT_IDS)
def test_float_cases_against_fp64(ecm, name, seed, shape, C, lam, sc, T, share):
    d, g, conf = float_case(seed, shape, C, sc, share)
    yardstick(ecm, name, d, g, conf, lam, sc, T)
    ecm.ops.check_async_errors()


# ---- the tile edges -----------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(2, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 3)]
EDGE_SHAPES += [(1, h, w) for h in (LINES - 1, LINES, LINES + 1) for w in (CHUNK - 1, CHUNK, CHUNK + 1)]
EDGE_SHAPES += [(1, 2 * LINES + 1, 2 * CHUNK + 1)]
EDGE_SHAPES += [(1, h, w) for h in (VCHUNK - 1, VCHUNK, VCHUNK + 1) for w in (VLINES - 1, VLINES, VLINES + 1)]
EDGE_SHAPES += [(1, 2 * VCHUNK + 1, 2 * VLINES + 1), (2, 2 * CHUNK + 1, 2 * LINES + 1)]
EDGE_SHAPES = list(dict.fromkeys(EDGE_SHAPES))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=["x".join(map(str, s)) for s in EDGE_SHAPES])
def test_tile_edges_against_fp64(ecm, shape):
    assert max(shape[1:]) <= 300
    B, H, W = shape
    gen = torch.Generator().manual_seed(H * 1000 + W)
    d = 5 + 30 * torch.rand(shape, generator=gen)
    g = 0.1 * torch.rand(B, 1, H, W, generator=gen) + 0.5 * (torch.arange(W) >= W // 2).float().view(1, 1, 1, W)
    conf = sparse_conf(shape, H * 1000 + W + 1, 0.3)
    conf[:, 0, 0] = 0.5                                                # at least one confident pixel per image
    yardstick(ecm, "edge_" + "x".join(map(str, shape)), d, g, conf, 64.0, 0.25, 2)
    ecm.ops.check_async_errors()


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
SHAPE_X = (2, LINES + 3, CHUNK + 7)


def smooth_guide(shape, seed, C=3):
    B, H, W = shape
    return 0.05 * torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed))


def test_a_constant_plane_comes_back_bit_for_bit(ecm):
    d = torch.full(SHAPE_X, 16.0)
    g = smooth_guide(SHAPE_X, 1)
    g[:, :, :, 40] = NAN                                               # and a cut: right of it nothing is confident below
    rand = sparse_conf(SHAPE_X, 2, 0.3)
    binary = (rand > 0).float()
    left_only = rand.clone()
    left_only[..., 40:] = 0
    for name, conf in (("none", None), ("random", rand), ("binary", binary), ("left_only", left_only)):
        s, w, w64 = yardstick(ecm, "const16_" + name, d, g, conf, 256.0, 0.25, 3)
        assert bool(((s == 16.0) | (s == 0)).all()) and torch.equal(s == 0, w64 == 0) and torch.equal(w == 0, w64 == 0)
        if name == "left_only":
            assert bool((s[..., 40:] == 0).all()) and bool((w[..., 40:] == 0).all()) and bool((s[..., :40] == 16.0).all())
        if name == "none":
            assert bool((s == 16.0).all())
    zero = ecm.ops.disparity_wls(d.to(DEV), g.to(DEV), torch.zeros(SHAPE_X, device=DEV), with_weight=True)
    assert all(bool((o == 0).all()) for o in zero)                     # nothing confident: all 0
    ecm.ops.check_async_errors()


def test_a_single_confident_pixel(ecm):
    B, H, W = shape = (1, 2 * LINES + 1, 2 * CHUNK + 1)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (LINES - 1, CHUNK - 1), (LINES, CHUNK), (VCHUNK, VLINES - 1)]
    d = 5 + 30 * torch.rand(shape, generator=torch.Generator().manual_seed(3))
    g = smooth_guide(shape, 4).to(DEV)
    for y, x in spots:
        dd, conf = d.clone(), torch.zeros(shape)
        dd[0, y, x], conf[0, y, x] = 4.0, 0.75
        s, w = ecm.ops.disparity_wls(dd.to(DEV), g, conf.to(DEV), 8000.0, 0.25, 3, with_weight=True)
        assert bool((w > 0).all()) and bool((s == 4.0).all()), (y, x)
    # a NaN column of the guide beside it: the far side hears nothing, the near side all of it
    y, x = LINES, CHUNK
    cut = g.clone()
    cut[:, :, :, x + 1] = NAN
    dd, conf = d.clone(), torch.zeros(shape)
    dd[0, y, x], conf[0, y, x] = 4.0, 0.75
    s, w = ecm.ops.disparity_wls(dd.to(DEV), cut, conf.to(DEV), 8000.0, 0.25, 3, with_weight=True)
    assert bool((w[..., :x + 1] > 0).all()) and bool((s[..., :x + 1] == 4.0).all())
    assert bool((s[..., x + 1:] == 0).all()) and bool((w[..., x + 1:] == 0).all())
    ecm.ops.check_async_errors()


def test_planted_non_finite_values(ecm):
    shape = SHAPE_X
    B, H, W = shape
    gen = torch.Generator().manual_seed(5)
    d = 5 + 30 * torch.rand(shape, generator=gen)
    g = smooth_guide(shape, 6)
    conf = sparse_conf(shape, 7, 0.5)
    spots = sorted({(0, 0), (H - 1, W - 1), (H // 2, W // 2), (LINES - 1, CHUNK - 1), (LINES, CHUNK), (0, W - 1), (H - 1, 0)})
    for i, (y, x) in enumerate(spots):
        d[B - 1, y, x] = (NAN, INF, -INF)[i % 3]
        conf[0, y, x] = (NAN, -1.0, -INF, INF)[i % 4]
    s, w, _ = yardstick(ecm, "planted", d, g, conf, 64.0, 0.25, 2)
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(w).all()) and bool((w >= 0).all())
    s, w, _ = yardstick(ecm, "planted_conf_none", d, g, None, 64.0, 0.25, 2)
    assert bool(torch.isfinite(s).all()) and bool((w > 0).all())
    ecm.ops.check_async_errors()


# ---- the op's contract --------------------------------------------------------------------------------------------------------------------
def test_reproducible_and_batch_independent(ecm):
    ops = ecm.ops
    shape = (2, 2 * LINES + 5, 2 * CHUNK + 9)
    gen = torch.Generator().manual_seed(8)
    d = (5 + 30 * torch.rand(shape, generator=gen)).to(DEV)
    g = torch.rand(2, 3, *shape[1:], generator=gen).to(DEV)
    conf = sparse_conf(shape, 9, 0.3).to(DEV)
    first = ops.disparity_wls(d, g, conf, 8000.0, 0.25, 3, with_weight=True)
    again = ops.disparity_wls(d, g, conf, 8000.0, 0.25, 3, with_weight=True)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    for b in range(2):
        one = ops.disparity_wls(d[b:b + 1], g[b:b + 1], conf[b:b + 1], 8000.0, 0.25, 3, with_weight=True)
        assert all(same_bits(a[0], f[b]) for a, f in zip(one, first))
    assert same_bits(ops.disparity_wls(d, g, conf, 8000.0, 0.25, 3), first[0])
    assert same_bits(ops.disparity_wls(d.unsqueeze(1), g, conf.unsqueeze(1), 8000.0, 0.25, 3), first[0])
    for as_mask in (torch.bool, torch.uint8):
        got = ops.disparity_wls(d, g, (conf > 0).to(as_mask), 8000.0, 0.25, 3, with_weight=True)
        want = ops.disparity_wls(d, g, (conf > 0).float(), 8000.0, 0.25, 3, with_weight=True)
        assert all(same_bits(a, b) for a, b in zip(got, want))
    assert same_bits(ops.disparity_wls(d, g), ops.disparity_wls(d, g, None, 8000.0, 0.25, 3))
    assert not ops.disparity_wls(d.clone().requires_grad_(), g, conf).requires_grad
    with pytest.raises(RuntimeError, match="confidence"):
        ops.disparity_wls(d, g, conf[:, :, :-1])
    with pytest.raises(RuntimeError, match="confidence"):
        ops.disparity_wls(d, g, conf.double())
    with pytest.raises(RuntimeError, match="guide"):
        ops.disparity_wls(d, g[:, :, :-1])
    with pytest.raises(RuntimeError, match="guide"):
        ops.disparity_wls(d, torch.zeros(2, 5, *shape[1:], device=DEV))
    ops.check_async_errors()


def test_guard_bands(ecm):
    shape = (2, LINES + 1, CHUNK + 7)
    gen = torch.Generator().manual_seed(10)
    d = (5 + 30 * torch.rand(shape, generator=gen)).to(DEV)
    conf = sparse_conf(shape, 11, 0.3).to(DEV)
    for C, c, T in ((3, conf, 3), (1, None, 1), (4, conf, 2)):
        g = torch.rand(2, C, *shape[1:], generator=gen).to(DEV)
        before = [t.clone() for t in (d, conf, g)]
        with guarded(ecm) as gb:
            ecm.ops.disparity_wls(d, g, c, 64.0, 0.25, T, with_weight=True)
            gb.check(f"disparity_wls C {C} T {T}")
            assert len(gb.records) == 2                                # out, and the scratch
        assert all(same_bits(a, b) for a, b in zip(before, (d, conf, g)))        # the inputs are not written
    ecm.ops.check_async_errors()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["cmfsm", "cmfsm_sub_8"])
def test_smooth_256x256(ecm, arch):
    H, W = 256, 256                    # the smallest frame both nets accept (tests/test_hip_disp_filter.py)
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    left, right = torch.randn(1, 3, H, W, device=DEV, generator=gen), torch.randn(1, 3, H, W, device=DEV, generator=gen)
    kw = dict(threshold=1.0, rel=0.05)
    cc = model.cross_check(left, right, **kw)
    out = model.smooth(left, right, speckle_size=50, speckle_diff=0.5, lam=512.0, sigma_color=1.5, iterations=2, **kw)
    assert type(out).__name__ == "Smoothed" and out._fields == cc._fields + ("confidence", "smoothed")
    assert all(f.shape == (1, 1, H, W) and not f.requires_grad for f in out)
    assert out.confidence.dtype == torch.float32 and out.smoothed.dtype == torch.float32
    assert all(same_bits(a, b) for a, b in zip(out[:5], cc))
    _, _, size = ops.disparity_speckle(cc.disparity, cc.kind == 0, 50, 0.5, with_segments=True)
    confidence = ((cc.kind[:, 0] == 0) & (size > 50)).float()
    assert torch.equal(out.confidence[:, 0], confidence)
    assert same_bits(out.smoothed[:, 0], ops.disparity_wls(cc.disparity, left, confidence, 512.0, 1.5, 2))
    assert bool(torch.isfinite(out.smoothed).all())
    # speckle_size=None: the consistent pixels alone
    plain = model.smooth(left, right, speckle_size=None, lam=512.0, sigma_color=1.5, iterations=2, **kw)
    confidence = (cc.kind[:, 0] == 0).float()
    assert all(same_bits(a, b) for a, b in zip(plain[:5], cc)) and torch.equal(plain.confidence[:, 0], confidence)
    assert same_bits(plain.smoothed[:, 0], ops.disparity_wls(cc.disparity, left, confidence, 512.0, 1.5, 2))
    # the defaults
    default = model.smooth(left, right)
    cc0 = model.cross_check(left, right)
    _, _, size = ops.disparity_speckle(cc0.disparity, cc0.kind == 0, 200, 1.0, with_segments=True)
    confidence = ((cc0.kind[:, 0] == 0) & (size > 200)).float()
    assert torch.equal(default.confidence[:, 0], confidence)
    assert same_bits(default.smoothed[:, 0], ops.disparity_wls(cc0.disparity, left, confidence))
    ops.check_async_errors()
