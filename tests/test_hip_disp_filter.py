"""The disparity post-filters on the MI355X: ops.disparity_median, ops.disparity_bilateral and
_ECMNet.refine against median_t and bilateral_t, the torch restatements of tests/test_disp_filter_cpu.py, in fp64 on the CPU.

Median: bit for bit, support included.  The values are random multiples of 1/4 in [0, 40) (ties abound), every radius, at
[2,1,1], [1,2,3], [1,3,63], [2,2,64], [1,2,65], one pixel less than / exactly / one pixel more than a tile, two tiles and a pixel
each way, and [1, GRID TH + 1, 7] (more tiles than the launch has workgroups), the tile read from csrc/disp_filter.hip.  The masks:
none; all ones; all zeros; a single usable pixel at each corner; a checkerboard; invalid runs of width 2r straddling every
tile edge in x and in y; NaN, +inf and -inf planted in d.

Bilateral: the project's yardstick of sections 14-17, max|out - out64| <= 4 e32 + 2e-7 max|out64|, e32 the error of the fp32
restatement run on the device, for `refined` and for `weight`, on test_disp_filter_cpu.FLOAT_CASES (which that file shows to be
comparable with fp64: no weight underflows).  Prints `DFRATIO <case> <ratio>`; section 18 records the worst.  Exact cases --
a constant d, nothing valid, a single usable pixel, each a power of two so that sum(w d) / sum(w) is exact -- bit for bit."""
import pytest
import torch

from test_disp_filter_cpu import FLOAT_CASES, FLOAT_IDS, FLOOR, K, KC, bilateral_t, float_case, median_t
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
TW, TH, GRID = KC["TW"], KC["TH"], KC["GRID"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


# ---- the median ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1, 1), (1, 2, 3), (1, 3, 63), (2, 2, 64), (1, 2, 65), (1, TH - 1, TW - 1), (1, TH, TW), (1, TH + 1, TW + 1),
          (1, 2 * TH + 1, 2 * TW + 1), (1, GRID * TH + 1, 7)]


def quarter_plane(shape, seed):
    return torch.randint(0, 160, shape, generator=torch.Generator().manual_seed(seed)).float() / 4


def masks(shape, r):
    """name -> (valid or None, the positions of d to overwrite: [(index, value)])."""
    B, H, W = shape
    y, x = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    full = lambda m: m.expand(B, H, W).contiguous()                                              # noqa: E731
    out = {"none": (None, []), "ones": (torch.ones(shape, dtype=torch.uint8), []), "zeros": (torch.zeros(shape, dtype=torch.bool), []),
           "checkerboard": (full((y + x) % 2 == 0), [])}
    for name, (cy, cx) in {"corner00": (0, 0), "corner01": (0, W - 1), "corner10": (H - 1, 0), "corner11": (H - 1, W - 1)}.items():
        out[name] = (full((y == cy) & (x == cx)).to(torch.uint8) * 255, [])
    runs = torch.ones(H, W, dtype=torch.bool)
    for p in range(TW, W + r, TW):
        runs[:, max(p - r, 0):p + r] = False
    for p in range(TH, H + r, TH):
        runs[max(p - r, 0):p + r, :] = False
    out["runs"] = (full(runs), [])
    spots = sorted({(0, 0), (H - 1, W - 1), (H // 2, W // 2), (min(TH, H) - 1, min(TW, W) - 1), (min(TH, H - 1), min(TW, W - 1)),
                    (0, W - 1), (H - 1, 0)})
    out["planted"] = (None, [((B - 1, yy, xx), (NAN, INF, -INF)[i % 3]) for i, (yy, xx) in enumerate(spots)])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_median_bit_for_bit(ecm, shape):
    assert SHAPES[-1][1] > GRID * TH and ecm.ops.disp_filter_max_radius("median") == 3
    for r in (1, 2, 3):
        for name, (valid, planted) in masks(shape, r).items():
            d = quarter_plane(shape, 100 * r + len(name))
            for at, value in planted:
                d[at] = value
            want = median_t(d.double(), valid, r)
            got = ecm.ops.disparity_median(d.to(DEV), None if valid is None else valid.to(DEV), r, with_support=True)
            for what, g, w in zip(("median", "support"), got, want):
                assert g.shape == d.shape and g.dtype == torch.float32
                bad = (g.cpu().double() != w).nonzero()
                assert bad.numel() == 0, f"{shape} r {r} {name}: {what} differs at {bad[:4].tolist()}: " \
                                         f"{g.cpu()[tuple(bad[0])]} != {w[tuple(bad[0])]}"
            if name == "planted":
                assert bool(torch.isfinite(got[0]).all())
    ecm.ops.check_async_errors()


# ---- the bilateral filter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,shape,C,r,ss,sc", FLOAT_CASES, ids=FLOAT_IDS)
def test_bilateral_float_cases(ecm, name, seed, shape, C, r, ss, sc):
    d, valid, g = float_case(seed, shape, C)
    want = bilateral_t(d.double(), valid, g.double(), r, ss, sc)
    dd, vd, gd = d.to(DEV), valid.to(DEV), g.to(DEV)
    plain = bilateral_t(dd, vd, gd, r, ss, sc)
    got = ecm.ops.disparity_bilateral(dd, gd, vd, r, ss, sc, with_weight=True)
    worst = 0.0
    for what, o, o32, o64 in zip(("refined", "weight"), got, plain, want):
        e32 = float((o32.cpu().double() - o64).abs().max())
        bound = K * e32 + FLOOR * float(o64.abs().max())
        err = float((o.cpu().double() - o64).abs().max())
        ratio = err / bound
        worst = max(worst, ratio)
        print(f"DFRATIO {name} {what} {ratio:.3f}   # err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name}: {what}: |hip - fp64| = {err:.3e} > {bound:.3e} (ratio {ratio:.2f})"
        assert torch.equal(o.cpu() == 0, o64 == 0)
    print(f"DFRATIO {name} {worst:.3f}")
    ecm.ops.check_async_errors()


@pytest.mark.parametrize("shape,C,r", [((2, 9, 200), 3, 4), ((1, 7, 130), 1, KC["R_MAX"]), ((1, TH + 1, 2 * TW + 1), 4, 2), ((1, 1, 1), 2, 1)])
def test_bilateral_exact_cases(ecm, shape, C, r):
    B, H, W = shape
    gen = torch.Generator().manual_seed(H * W + r)
    g = torch.rand(B, C, H, W, generator=gen)
    valid = torch.rand(B, H, W, generator=gen) >= 0.3
    ss, sc = r / 2 + 0.5, 0.5
    run = lambda d, v: ecm.ops.disparity_bilateral(d.to(DEV), g.to(DEV), None if v is None else v.to(DEV), r, ss, sc, with_weight=True)   # noqa: E731
    # a constant d: 16 w is exact, so sum(16 w) is 16 sum(w) whatever the order, and the quotient is 16
    const = torch.full(shape, 16.0)
    for v in (None, valid):
        refined, weight = run(const, v)
        want, w64 = bilateral_t(const.double(), v, g.double(), r, ss, sc)
        assert torch.equal(refined.cpu().double(), want) and bool(((want == 16) | (want == 0)).all())
        assert torch.equal(weight.cpu() > 0, w64 > 0)
    # nothing valid
    refined, weight = run(const, torch.zeros(shape, dtype=torch.bool))
    assert bool((refined == 0).all()) and bool((weight == 0).all())
    # a single usable pixel: 4 over its window, 0 elsewhere, and the weight of the centre is exp(0)
    for y0, x0 in ((0, 0), (H - 1, W - 1), (H // 2, min(TW, W - 1))):
        lone = torch.zeros(shape, dtype=torch.bool)
        lone[B - 1, y0, x0] = True
        d = torch.full(shape, 4.0)
        d[valid] = 7.0                                                 # what must not be read
        d[B - 1, y0, x0] = 4.0
        refined, weight = run(d, lone)
        want, w64 = bilateral_t(d.double(), lone, g.double(), r, ss, sc)
        assert torch.equal(refined.cpu().double(), want) and float(weight[B - 1, y0, x0]) == 1.0
        assert torch.equal(weight.cpu() > 0, w64 > 0) and int((want == 4).sum()) == int((w64 > 0).sum())
    ecm.ops.check_async_errors()


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_bilateral_non_finite_inputs(ecm, bad):
    shape, C, r, ss, sc = (1, TH + 2, TW + 5), 3, 3, 2.0, 0.5
    d, valid, g = float_case(9, shape, C)
    g = g * 0.5
    for yy, xx in ((0, 0), (TH - 1, TW - 1), (TH, TW), (3, 7)):
        d[0, yy, xx] = bad
    g[0, 1, 2, 9] = bad
    g[0, 0, TH, TW + 1] = NAN
    want = bilateral_t(d.double(), valid, g.double(), r, ss, sc)
    plain = bilateral_t(d.to(DEV), valid.to(DEV), g.to(DEV), r, ss, sc)
    got = ecm.ops.disparity_bilateral(d.to(DEV), g.to(DEV), valid.to(DEV), r, ss, sc, with_weight=True)
    for o, o32, o64 in zip(got, plain, want):
        assert bool(torch.isfinite(o).all())
        bound = K * float((o32.cpu().double() - o64).abs().max()) + FLOOR * float(o64.abs().max())
        assert float((o.cpu().double() - o64).abs().max()) <= bound
    assert float(got[1][0, TH, TW + 1]) == 0 and float(got[0][0, TH, TW + 1]) == 0          # a NaN guide at the centre: nothing is left
    ecm.ops.check_async_errors()


# ---- the ops' contract -----------------------------------------------------------------------------------------------------------------
def test_shapes_strides_and_streams(ecm):
    ops = ecm.ops
    d, valid, g = (t.to(DEV) for t in float_case(7, (2, 6, 130), 3))
    med = ops.disparity_median(d, valid, 2, with_support=True)
    bil = ops.disparity_bilateral(d, g, valid, 3, with_weight=True)
    assert len(med) == 2 and len(bil) == 2 and ops.disparity_median(d).shape == d.shape and ops.disparity_bilateral(d, g).shape == d.shape
    same = lambda got, want: all(torch.equal(a, b) for a, b in zip(got, want))                  # noqa: E731
    assert same(ops.disparity_median(d.unsqueeze(1), valid.unsqueeze(1), 2, with_support=True), med)
    assert same(ops.disparity_median(d, valid.to(torch.uint8) * 3, 2, with_support=True), med)
    assert same(ops.disparity_bilateral(d.unsqueeze(1), g, valid.to(torch.uint8), 3, with_weight=True), bil)
    wide, tall = torch.zeros(2, 6, 260, device=DEV), torch.zeros(2, 3, 130, 6, device=DEV)
    wide[:, :, ::2], tall[:] = d, g.transpose(2, 3)
    nd, ng, nv = wide[:, :, ::2], tall.transpose(2, 3), valid.transpose(1, 2).contiguous().transpose(1, 2)
    assert not nd.is_contiguous() and not ng.is_contiguous() and not nv.is_contiguous()
    assert same(ops.disparity_median(nd, nv, 2, with_support=True), med) and same(ops.disparity_bilateral(nd, ng, nv, 3, with_weight=True), bil)
    assert same(ops.disparity_bilateral(d.clone().requires_grad_(), g, valid, 3, with_weight=True), bil) and not bil[0].requires_grad
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.disparity_median(d, valid, 2, with_support=True) + ops.disparity_bilateral(d, g, valid, 3, with_weight=True)
    side.synchronize()
    assert same(got, med + bil)
    with pytest.raises(RuntimeError, match="valid"):
        ops.disparity_median(d, valid[:, :, :-1])
    with pytest.raises(RuntimeError, match="valid"):
        ops.disparity_median(d, valid.float())
    with pytest.raises(RuntimeError, match="guide"):
        ops.disparity_bilateral(d, g[:, :, :-1])
    with pytest.raises(RuntimeError, match="guide"):
        ops.disparity_bilateral(d, torch.cat([g, g], 1))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.disparity_median(d.double())
    with pytest.raises(ValueError, match="radius"):
        ops.disparity_median(d, radius=4)
    ops.check_async_errors()


def test_guard_bands(ecm):
    ops = ecm.ops
    d, valid, g = (t.to(DEV) for t in float_case(8, (2, TH + 3, TW + 7), 3))
    for r in (1, 2, 3):
        with guarded(ecm) as gb:
            ops.disparity_median(d, valid, r, with_support=True)
            gb.check(f"disparity_median r {r}")
            assert len(gb.records) == 1
    for r in (1, 5, KC["R_MAX"]):
        with guarded(ecm) as gb:
            ops.disparity_bilateral(d, g, valid, r, with_weight=True)
            gb.check(f"disparity_bilateral r {r}")
            assert len(gb.records) == 1
    ops.check_async_errors()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["cmfsm", "cmfsm_sub_8"])
def test_refine_256x256(ecm, arch):
    H, W = 256, 256                    # the smallest frame both nets accept: their widest pyramid pool needs a 64 x 64 (1/4) or 32 x 32 (1/8) map
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    left, right = torch.randn(1, 3, H, W, device=DEV, generator=gen), torch.randn(1, 3, H, W, device=DEV, generator=gen)
    cc = model.cross_check(left, right, threshold=1.0, rel=0.05)
    out = model.refine(left, right, threshold=1.0, rel=0.05)
    assert type(out).__name__ == "Refined" and all(f.shape == (1, 1, H, W) and not f.requires_grad for f in out)
    assert all(torch.equal(a, b) for a, b in zip(out[:5], cc))
    median = ops.disparity_median(cc.filled, cc.filled > 0, 2)
    refined = ops.disparity_bilateral(median, left, median > 0, 4, 2.0, 0.25)
    assert torch.equal(out.median[:, 0], median) and torch.equal(out.refined[:, 0], refined)
    assert bool(torch.isfinite(out.refined).all()) and bool((out.refined >= 0).all())
    other = model.refine(left, right, threshold=1.0, rel=0.05, median_radius=None, bilateral_radius=2, sigma_space=1.0, sigma_color=0.5)
    assert torch.equal(other.median, cc.filled)
    assert torch.equal(other.refined[:, 0], ops.disparity_bilateral(cc.filled, left, cc.filled > 0, 2, 1.0, 0.5))
    other = model.refine(left, right, threshold=1.0, rel=0.05, median_radius=3, bilateral_radius=None)
    assert torch.equal(other.median[:, 0], ops.disparity_median(cc.filled, cc.filled > 0, 3)) and torch.equal(other.refined, other.median)
    other = model.refine(left, right, threshold=1.0, rel=0.05, median_radius=None, bilateral_radius=None)
    assert torch.equal(other.median, cc.filled) and torch.equal(other.refined, cc.filled)
    ops.check_async_errors()
