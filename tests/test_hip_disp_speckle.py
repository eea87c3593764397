"""The speckle filter on the MI355X: ops.disparity_speckle and _ECMNet.despeckle against speckle_t, the
sequential union-find of tests/test_disp_speckle_cpu.py.  Everything is compared bit for bit: out, label and size.

The values are random multiples of 1/4 in [0, 4) and max_diff is 0, 0.25 or 1.0, so merges are frequent and the inclusive
boundary falls on exact fp32 values; max_size is 0, 1, 5 or 10^6.  label and size do not depend on max_size, so the reference
labels one input once per max_diff.  Shapes: [2,1,1], [1,2,3], [1,3,63], [2,2,64], [1,2,65], one pixel less than / exactly / one
pixel more than a tile, two tiles and a pixel, four tiles and two pixels each way, and [1, GRID TH + 1, 3] (more tiles than the
launch has workgroups), the tile read from csrc/disp_speckle.hip.  Masks: none; all ones; all zeros; a single usable pixel at each
corner; a checkerboard; 30 % random; NaN, +inf and -inf planted in d.  Structured inputs whose segments cross tile borders have
closed forms as well."""
import numpy as np
import pytest
import torch

from test_disp_speckle_cpu import KC, removed_t, same_bits, segments_t, speckle_t
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
TW, TH, GRID = KC["TW"], KC["TH"], KC["GRID"]
NAN, INF = float("nan"), float("inf")
MAX_DIFFS, MAX_SIZES = (0.0, 0.25, 1.0), (0, 1, 5, 10 ** 6)


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def quarter_plane(shape, seed):
    return torch.randint(0, 16, shape, generator=torch.Generator().manual_seed(seed)).float() / 4


def compare(ecm, d, valid, max_diffs=MAX_DIFFS, max_sizes=MAX_SIZES, what=""):
    """The op against speckle_t for every max_diff and max_size; returns {max_diff: (label, size)} of the reference."""
    dd, vd = d.to(DEV), None if valid is None else valid.to(DEV)
    refs = {}
    for max_diff in max_diffs:
        label, size = refs[max_diff] = segments_t(d, valid, max_diff)
        for max_size in max_sizes:
            out, got_label, got_size = ecm.ops.disparity_speckle(dd, vd, max_size, max_diff, with_segments=True)
            assert out.shape == d.shape and out.dtype == torch.float32
            assert got_label.shape == d.shape and got_label.dtype == torch.int32 and got_size.dtype == torch.int32
            where = f"{what} {tuple(d.shape)} max_diff {max_diff} max_size {max_size}"
            for name, got, want in (("label", got_label, label), ("size", got_size, size)):
                bad = (got.cpu() != torch.from_numpy(want)).nonzero()
                assert bad.numel() == 0, f"{where}: {name} differs at {bad[:4].tolist()}: " \
                                         f"{got.cpu()[tuple(bad[0])]} != {want[tuple(bad[0].tolist())]}"
            assert same_bits(out.cpu(), torch.from_numpy(removed_t(d, size, max_size))), f"{where}: out differs"
    return refs


# ---- random planes at every tile edge ---------------------------------------------------------------------------------------------------
SHAPES = [(2, 1, 1), (1, 2, 3), (1, 3, 63), (2, 2, 64), (1, 2, 65), (1, TH - 1, TW - 1), (1, TH, TW), (1, TH + 1, TW + 1),
          (1, 2 * TH + 1, 2 * TW + 1), (1, 4 * TH + 1, 2 * TW + 2), (1, GRID * TH + 1, 3)]


def masks(shape):
    """name -> (valid or None, the positions of d to overwrite: [(index, value)])."""
    B, H, W = shape
    y, x = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    full = lambda m: m.expand(B, H, W).contiguous()                                              # noqa: E731
    out = {"none": (None, []), "ones": (torch.ones(shape, dtype=torch.uint8), []), "zeros": (torch.zeros(shape, dtype=torch.bool), []),
           "checkerboard": (full((y + x) % 2 == 0), []),
           "random": (torch.rand(shape, generator=torch.Generator().manual_seed(H * W)) >= 0.3, [])}
    for name, (cy, cx) in {"corner00": (0, 0), "corner01": (0, W - 1), "corner10": (H - 1, 0), "corner11": (H - 1, W - 1)}.items():
        out[name] = (full((y == cy) & (x == cx)).to(torch.uint8) * 255, [])
    spots = sorted({(0, 0), (H - 1, W - 1), (H // 2, W // 2), (min(TH, H) - 1, min(TW, W) - 1), (min(TH, H - 1), min(TW, W - 1)),
                    (0, W - 1), (H - 1, 0)})
    out["planted"] = (None, [((B - 1, yy, xx), (NAN, INF, -INF)[i % 3]) for i, (yy, xx) in enumerate(spots)])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bit_for_bit(ecm, shape):
    assert SHAPES[-1][1] > GRID * TH
    for name, (valid, planted) in masks(shape).items():
        d = quarter_plane(shape, 7 + len(name))
        for at, value in planted:
            d[at] = value
        refs = compare(ecm, d, valid, what=name)
        if name == "zeros":
            assert all((label == -1).all() and (size == 0).all() for label, size in refs.values())
    ecm.ops.check_async_errors()


# ---- segments that cross tile borders -------------------------------------------------------------------------------------------------
H2, W2 = 2 * TH + 3, 2 * TW + 5                                        # 3 x 3 tiles, the last row and column of them ragged


def serpentine(H, W):
    """A one-pixel path through every even row, the rows joined alternately at the right and at the left end."""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def test_serpentines(ecm):
    for name, path in (("rows", serpentine(H2, W2)), ("columns", serpentine(W2, H2).t().contiguous())):
        # as a mask over a constant plane, and as a plane of two values 2 apart (the rest is then segments of its own)
        flat, two = torch.full((1, H2, W2), 1.25), torch.where(path, 1.25, 3.25).view(1, H2, W2)
        n = int(path.sum())
        refs = compare(ecm, flat, path.view(1, H2, W2), (0.0,), (0, n - 1, n), what=f"serpentine {name} mask")
        label, size = refs[0.0]
        assert (size[0][path.numpy()] == n).all() and (label[0][path.numpy()] == 0).all() and (size[0][~path.numpy()] == 0).all()
        refs = compare(ecm, two, None, (1.0,), (0, n - 1, n), what=f"serpentine {name} values")
        assert (refs[1.0][1][0][path.numpy()] == n).all()
    ecm.ops.check_async_errors()


def test_u_comb_and_constant(ecm):
    d = quarter_plane((1, H2, W2), 3)
    # a U: two arms in the first tile that join only in the tile below it
    u = torch.zeros(H2, W2, dtype=torch.bool)
    u[0:TH + 2, 3] = u[0:TH + 2, 10] = True
    u[TH + 1, 3:11] = True
    refs = compare(ecm, torch.full((1, H2, W2), 2.0), u.view(1, H2, W2), (0.0,), (0, 10 ** 6), what="U")
    assert (refs[0.0][0][0][u.numpy()] == 3).all() and (refs[0.0][1][0][u.numpy()] == int(u.sum())).all()
    # a comb: a spine along the last row, teeth on every other column up through all the tiles above
    comb = torch.zeros(H2, W2, dtype=torch.bool)
    comb[H2 - 1] = True
    comb[:, 0::2] = True
    refs = compare(ecm, torch.full((1, H2, W2), 2.0), comb.view(1, H2, W2), (0.0,), (0, 10 ** 6), what="comb")
    assert (refs[0.0][0][0][comb.numpy()] == 0).all() and (refs[0.0][1][0][comb.numpy()] == int(comb.sum())).all()
    # the same comb as values: the gaps between the teeth are segments too
    compare(ecm, torch.where(comb, 2.0, 3.5).view(1, H2, W2), None, (0.0, 1.0), (0, 5), what="comb values")
    # a constant plane: one segment per image, every border pair joined
    refs = compare(ecm, torch.full((2, H2, W2), 0.75), None, (0.0,), (0, H2 * W2 - 1, H2 * W2), what="constant")
    assert (refs[0.0][0] == 0).all() and (refs[0.0][1] == H2 * W2).all()
    # ramps along x and along y whose step is max_diff: one segment across every border, the ends far apart
    x = torch.arange(W2).float().view(1, 1, W2).expand(1, H2, W2) * 0.25
    y = torch.arange(H2).float().view(1, H2, 1).expand(1, H2, W2) * 0.25
    for ramp in (x + 0 * d, x + 100 * y, y + 100 * x):
        compare(ecm, ramp.contiguous(), None, (0.25, 0.2499), (0, 5), what="ramp")
    ecm.ops.check_async_errors()


def test_tile_corners(ecm):
    # two 3 x 3 blobs that meet only diagonally, at the corner where four tiles meet: they stay apart
    m = torch.zeros(H2, W2, dtype=torch.bool)
    m[TH - 3:TH, TW - 3:TW] = True
    m[TH:TH + 3, TW:TW + 3] = True
    refs = compare(ecm, torch.full((1, H2, W2), 1.0), m.view(1, H2, W2), (0.0, 1.0), (0, 8, 9), what="diagonal")
    label, size = refs[0.0]
    assert (size[0][m.numpy()] == 9).all() and label[0, TH - 1, TW - 1] == (TH - 3) * W2 + TW - 3 and label[0, TH, TW] == TH * W2 + TW
    # the same with the other diagonal, as values on a far background
    d = torch.full((1, H2, W2), 3.5)
    d[0, TH - 3:TH, TW:TW + 3] = 1.0
    d[0, TH:TH + 3, TW - 3:TW] = 1.0
    refs = compare(ecm, d, None, (1.0,), (0, 9), what="diagonal values")
    assert refs[1.0][1][0, TH - 1, TW] == 9 and refs[1.0][1][0, TH, TW - 1] == 9
    # a segment of exactly max_size pixels and one of max_size + 1, each in all four tiles about a corner
    k = 4
    d = torch.full((1, H2, W2), 3.5)
    d[0, TH - 1:TH + 1, TW - 1:TW + 1] = 1.0                           # 2 x 2 = k pixels
    d[0, 2 * TH - 1:2 * TH + 1, 2 * TW - 1:2 * TW + 1] = 1.0           # 2 x 2 and one more
    d[0, 2 * TH + 1, 2 * TW] = 1.0
    compare(ecm, d, None, (1.0,), (k - 1, k, k + 1), what="max_size")
    out, _, size = ecm.ops.disparity_speckle(d.to(DEV), None, k, 1.0, with_segments=True)
    assert int(size[0, TH, TW]) == k and int(size[0, 2 * TH, 2 * TW]) == k + 1
    assert float(out[0, TH, TW]) == 0 and float(out[0, TH - 1, TW - 1]) == 0 and float(out[0, 2 * TH, 2 * TW]) == 1.0
    assert int((out == 0).sum()) == k
    ecm.ops.check_async_errors()


def test_many_tiles_and_images(ecm):
    """Dozens of tiles and three images: large winding segments, many concurrent unions on few roots."""
    shape = (3, 5 * TH + 3, 4 * TW + 9)
    d = quarter_plane(shape, 21)
    valid = torch.rand(shape, generator=torch.Generator().manual_seed(22)) >= 0.1
    compare(ecm, d, valid, (0.25, 1.0), (5, 200), what="many tiles")
    compare(ecm, torch.full(shape, 2.5), valid, (0.0,), (200,), what="many tiles, constant")
    ecm.ops.check_async_errors()


# ---- the op's contract ----------------------------------------------------------------------------------------------------------------
def test_op_behaviour(ecm):
    ops = ecm.ops
    shape = (2, TH + 3, TW + 7)
    d = quarter_plane(shape, 5).to(DEV)
    valid = (torch.rand(shape, generator=torch.Generator().manual_seed(6)) >= 0.3).to(DEV)
    same = lambda got, want: all(torch.equal(a, b) for a, b in zip(got, want))                  # noqa: E731
    first = ops.disparity_speckle(d, valid, 5, 0.25, with_segments=True)
    assert len(first) == 3 and same(ops.disparity_speckle(d, valid, 5, 0.25, with_segments=True), first)
    assert torch.equal(ops.disparity_speckle(d, valid, 5, 0.25), first[0])
    assert same(ops.disparity_speckle(d, valid.to(torch.uint8) * 3, 5, 0.25, with_segments=True), first)
    got = ops.disparity_speckle(d.unsqueeze(1), valid.unsqueeze(1), 5, 0.25, with_segments=True)
    assert all(g.shape == shape for g in got) and same(got, first)
    assert same(ops.disparity_speckle(d, valid, np.int64(5), 0.25, with_segments=True), first)
    wide = torch.zeros(2, TH + 3, 2 * (TW + 7), device=DEV)
    wide[:, :, ::2] = d
    assert not wide[:, :, ::2].is_contiguous() and same(ops.disparity_speckle(wide[:, :, ::2], valid, 5, 0.25, with_segments=True), first)
    assert not ops.disparity_speckle(d.clone().requires_grad_(), valid, 5, 0.25).requires_grad
    default = ops.disparity_speckle(d)
    assert torch.equal(default, ops.disparity_speckle(d, None, 200, 1.0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.disparity_speckle(d, valid, 5, 0.25, with_segments=True)
    side.synchronize()
    assert same(got, first)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_speckle(d.cpu())
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_speckle(d, valid.cpu())
    with pytest.raises(RuntimeError, match="valid"):
        ops.disparity_speckle(d, valid[:, :, :-1])
    with pytest.raises(RuntimeError, match="valid"):
        ops.disparity_speckle(d, valid.float())
    with pytest.raises(RuntimeError, match="want"):
        ops.disparity_speckle(d[0, 0])
    for kw, what in (({"max_size": -1}, "max_size"), ({"max_size": 1.5}, "max_size"), ({"max_size": True}, "max_size"),
                     ({"max_diff": -1.0}, "max_diff"), ({"max_diff": NAN}, "max_diff"), ({"max_diff": INF}, "max_diff")):
        with pytest.raises(ValueError, match=what):                    # before the tensor is looked at: a CPU tensor does not get as far
            ops.disparity_speckle(d.cpu(), **kw)
    ops.check_async_errors()


def test_guard_bands(ecm):
    shape = (2, 11, 71)
    d = quarter_plane(shape, 8).to(DEV)
    valid = (torch.rand(shape, generator=torch.Generator().manual_seed(9)) >= 0.3).to(DEV)
    for v, max_diff in ((valid, 0.25), (None, 1.0), (None, 0.0)):
        with guarded(ecm) as gb:
            ecm.ops.disparity_speckle(d, v, 5, max_diff, with_segments=True)
            gb.check(f"disparity_speckle max_diff {max_diff}")
            assert len(gb.records) == 2                                # out, and (label, size)
    ecm.ops.check_async_errors()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["cmfsm", "cmfsm_sub_8"])
def test_despeckle_256x256(ecm, arch):
    H, W = 256, 256                    # the smallest frame both nets accept (tests/test_hip_disp_filter.py)
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    left, right = torch.randn(1, 3, H, W, device=DEV, generator=gen), torch.randn(1, 3, H, W, device=DEV, generator=gen)
    kw = dict(threshold=1.0, rel=0.05)
    # speckle_size=None: refine itself
    plain = model.refine(left, right, **kw)
    none = model.despeckle(left, right, speckle_size=None, **kw)
    assert type(none).__name__ == "Refined" and type(none) is type(plain) and all(torch.equal(a, b) for a, b in zip(none, plain))
    cc = model.cross_check(left, right, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain[:5], cc))
    # speckle_size=50
    out = model.despeckle(left, right, speckle_size=50, speckle_diff=0.5, **kw)
    assert type(out).__name__ == "Despeckled" and out._fields == plain._fields + ("despeckled", "segment")
    assert all(f.shape == (1, 1, H, W) and not f.requires_grad for f in out)
    assert out.despeckled.dtype == torch.float32 and out.segment.dtype == torch.int32
    assert all(torch.equal(a, b) for a, b in zip(out[:5], cc))
    # by hand: the op on the checked map, then every pixel of `filled` with the fate of the column it was copied from
    kept, label, size = ops.disparity_speckle(cc.disparity, cc.kind == 0, 50, 0.5, with_segments=True)
    error, kind, filled, src = ops.lr_check(cc.disparity, cc.disparity_right, 1.0, 0.05, with_source=True)
    assert torch.equal(filled, cc.filled[:, 0]) and torch.equal(kind, cc.kind[:, 0])
    own = torch.arange(W, device=DEV, dtype=torch.int32).view(1, 1, W).expand(1, H, W)
    assert torch.equal(src[kind == 0], own[kind == 0])                 # a consistent pixel is its own source
    despeckled = torch.zeros_like(filled)
    take = (src >= 0) & (torch.gather(kept, 2, src.clamp(min=0).long()) > 0)
    despeckled[take] = filled[take]
    assert torch.equal(out.segment[:, 0], size) and torch.equal(out.despeckled[:, 0], despeckled)
    assert bool((out.segment[cc.kind != 0] == 0).all()) and bool((out.segment[cc.kind == 0] > 0).all())
    assert bool((out.despeckled[(cc.kind == 0) & (out.segment <= 50)] == 0).all())
    median = ops.disparity_median(despeckled, despeckled > 0, 2)
    refined = ops.disparity_bilateral(median, left, median > 0, 4, 2.0, 0.25)
    assert torch.equal(out.median[:, 0], median) and torch.equal(out.refined[:, 0], refined)
    assert bool(torch.isfinite(out.refined).all()) and bool((out.refined >= 0).all())
    # the segments of the model's map against the reference, once
    want = speckle_t(cc.disparity[:, 0].cpu(), (cc.kind[:, 0] == 0).cpu(), 50, 0.5)
    assert same_bits(kept.cpu(), want[0]) and torch.equal(label.cpu(), want[1]) and torch.equal(size.cpu(), want[2])
    # the None radii
    other = model.despeckle(left, right, median_radius=None, bilateral_radius=2, sigma_space=1.0, sigma_color=0.5, speckle_size=50,
                            speckle_diff=0.5, **kw)
    assert torch.equal(other.despeckled[:, 0], despeckled) and torch.equal(other.median, other.despeckled)
    assert torch.equal(other.refined[:, 0], ops.disparity_bilateral(despeckled, left, despeckled > 0, 2, 1.0, 0.5))
    other = model.despeckle(left, right, median_radius=3, bilateral_radius=None, speckle_size=50, speckle_diff=0.5, **kw)
    assert torch.equal(other.median[:, 0], ops.disparity_median(despeckled, despeckled > 0, 3)) and torch.equal(other.refined, other.median)
    other = model.despeckle(left, right, median_radius=None, bilateral_radius=None, speckle_size=0, **kw)
    assert torch.equal(other.median, other.despeckled) and torch.equal(other.refined, other.despeckled)
    assert torch.equal(other.despeckled, torch.where(cc.filled > 0, cc.filled, 0.0))      # max_size = 0 removes no segment
    ops.check_async_errors()
