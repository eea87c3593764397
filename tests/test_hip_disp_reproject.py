"""ops.disparity_reproject, ops.point_cloud and _ECMNet.point_cloud on the device against reproject_t and
cloud_t of tests/test_disp_reproject_cpu.py.  Everything the predicate and the compaction decide is compared bit for bit -- the
mask, the offsets, N, the pixel each row came from (its index travels as an attribute plane), the attribute columns, the zeros at
unusable dense pixels; the coordinates to the fp64 restatement rounded to fp32, within ONE fp32 ulp: the device evaluates the same
fp64 expression with a relative error of a few 2^-53, so the only way to another fp32 is a double-rounding straddle.  That holds
while nothing cancels in fp64, which `well_conditioned` asserts on every fixture matrix.  The shapes are the smallest at which a
rank can go wrong: one pixel, a width that is no multiple of the wave, exactly one tile, one tile plus a pixel, several tiles per
image with the last partial."""
import ctypes as C

import pytest
import torch

from test_disp_reproject_cpu import cloud_t, reproject_t, well_conditioned
import test_hip_abi_calls as abi_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def TILE(ecm):
    return ecm.ops.point_cloud_tile()


def shapes(TILE):
    return {"one_pixel": (1, 1, 1), "ragged": (2, 5, 67), "one_tile": (1, 64, TILE // 64), "tile_plus_one": (1, 1, TILE + 1),
            "several_tiles": (3, 33, 130)}


SHAPES = ("one_pixel", "ragged", "one_tile", "tile_plus_one", "several_tiles")


def matrices(ecm, B, H, W):
    """A shared matrix for B < 3, one per image otherwise; every one passes well_conditioned."""
    q = ecm.ops.q_matrix
    Q = q(711.3, 0.537, 0.37 * W + 0.123, 0.41 * H + 0.217, cx_right=0.37 * W + 1.123, x0=3, y0=2)
    if B >= 3:
        Q = torch.stack([Q, q(350.7, 0.12, 11.31, 7.77), q(1200.1, 1.9, 0.61 * W + 0.3, 0.2 * H + 0.45, x0=1)] +
                        [Q] * (B - 3))
    assert well_conditioned(Q, H, W)
    return Q


def disparity(B, H, W, seed, holes=True):
    """Positive disparities in (0.5, 190) with, where `holes`, a sprinkling of what the predicate must drop on its own: NaN, +-inf,
    0.0 (== min_disp), -0.0 and negative values."""
    g = torch.Generator().manual_seed(seed)
    d = 0.5 + 189.5 * torch.rand(B, H, W, generator=g)
    if holes:
        r = torch.rand(B, H, W, generator=g)
        for k, bad in enumerate((NAN, INF, -INF, 0.0, -0.0, -3.5)):
            d[(r >= 0.02 * k) & (r < 0.02 * (k + 1))] = bad
    return d


def pattern(name, B, H, W, TILE):
    """valid [B,H,W] bool."""
    n = H * W
    flat = torch.zeros(B, n, dtype=torch.bool)
    if name == "all":
        flat[:] = True
    elif name == "none":
        pass
    elif name == "middle_empty":
        flat[:] = True
        flat[B // 2] = False
    elif name == "runs":                     # runs across the wave borders at 64 and 256 (the next item) and across the tile border
        for lo, hi in ((50, 80), (250, 260), (TILE - 5, TILE + 5), (2 * TILE - 1, 2 * TILE + 70), (n - 3, n)):
            flat[:, max(lo, 0):max(min(hi, n), 0)] = True
    elif name.startswith("random"):
        share = float(name[6:])
        flat = torch.rand(B, n, generator=torch.Generator().manual_seed(int(share * 100) + n)) < share
    else:
        raise KeyError(name)
    return flat.view(B, H, W)


def ulps(a, b):
    """Distance in fp32 ulps between two finite fp32 tensors whose corresponding entries have one sign (or are equal)."""
    same = a == b
    assert bool((same | (torch.signbit(a) == torch.signbit(b))).all())
    return torch.where(same, 0, (a.view(torch.int32).long() - b.view(torch.int32).long()).abs())


EXACT = {"cases": 0, "not_bit_equal": 0}        # how often the coordinates were NOT bit-equal (DESIGN.md section 23 quotes it)


def run_and_check(ecm, d, Q, valid, C_, min_disp=0.0, max_disp=None, attributes=None):
    """ops.point_cloud(with_dense=True) and ops.disparity_reproject of the case against cloud_t; returns the device results."""
    B, H, W = d.shape
    if attributes is None and C_:
        index = torch.arange(B * H * W, dtype=torch.float32).view(B, 1, H, W)           # < 2^24: exact in fp32
        extra = torch.rand(B, C_ - 1, H, W, generator=torch.Generator().manual_seed(C_))
        attributes = torch.cat([index, extra], 1)
    want_points, want_offsets, want_xyz, want_mask, _ = cloud_t(d, Q, attributes, valid, min_disp, max_disp)
    dev = lambda t: None if t is None else t.to(DEV)                                     # noqa: E731
    got = ecm.ops.point_cloud(dev(d), Q, dev(attributes), dev(valid), min_disp, max_disp, with_dense=True)
    points, offsets, xyz, mask = (t.cpu() for t in got)
    assert mask.dtype == torch.bool and torch.equal(mask, want_mask)
    assert offsets.dtype == torch.int64 and torch.equal(offsets, want_offsets)
    assert points.shape == want_points.shape == (int(want_mask.sum()), 3 + C_) and points.dtype == torch.float32
    assert torch.equal(points[:, 3:].view(torch.int32), want_points[:, 3:].view(torch.int32))       # which pixel, and its attributes
    holes = ~want_mask.unsqueeze(1).expand(-1, 3, -1, -1)
    assert bool((xyz[holes].view(torch.int32) == 0).all())                                          # +0.0
    assert bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(want_xyz).all())
    worst = max(int(ulps(xyz, want_xyz).max()), int(ulps(points[:, :3], want_points[:, :3]).max()) if len(points) else 0)
    EXACT["cases"] += 1
    EXACT["not_bit_equal"] += worst != 0
    print(f"REPROJECT {tuple(d.shape)} C={C_} N={len(points)}: worst coordinate difference {worst} ulp")
    assert worst <= 1
    # the rows are the dense planes gathered at the mask, bit for bit
    b, y, x = mask.nonzero(as_tuple=True)
    assert torch.equal(points[:, :3].view(torch.int32), xyz[b, :, y, x].view(torch.int32))
    # the dense op alone writes the same planes
    xyz2, mask2 = ecm.ops.disparity_reproject(dev(d), Q, dev(valid), min_disp, max_disp, with_mask=True)
    assert torch.equal(xyz2.cpu().view(torch.int32), xyz.view(torch.int32)) and torch.equal(mask2.cpu(), mask)
    return got


@pytest.mark.parametrize("name", ["all", "none", "runs", "random0.1", "random0.9"])
@pytest.mark.parametrize("shape", SHAPES)
def test_patterns(ecm, TILE, shape, name):
    B, H, W = shapes(TILE)[shape]
    C_ = {"all": 1, "none": 3, "runs": 4, "random0.1": 1, "random0.9": 3}[name]
    d = disparity(B, H, W, seed=B * H + W, holes=name.startswith("random"))
    points, offsets, _, _ = run_and_check(ecm, d, matrices(ecm, B, H, W), pattern(name, B, H, W, TILE), C_)
    if name == "none":
        assert points.shape == (0, 3 + C_) and offsets.tolist() == [0] * (B + 1)
    if name == "all":
        assert offsets.tolist() == [b * H * W for b in range(B + 1)]


def test_only_the_middle_image_empty(ecm, TILE):
    B, H, W = shapes(TILE)["several_tiles"]
    _, offsets, _, _ = run_and_check(ecm, disparity(B, H, W, 5, holes=False), matrices(ecm, B, H, W), pattern("middle_empty", B, H, W, TILE), 1)
    assert offsets.tolist() == [0, H * W, H * W, 2 * H * W]


@pytest.mark.parametrize("shape", SHAPES)
def test_a_single_valid_pixel(ecm, TILE, shape):
    B, H, W = shapes(TILE)[shape]
    n = H * W
    d, Q = disparity(B, H, W, 9, holes=False), matrices(ecm, B, H, W)
    for at in sorted({0, n - 1, min(63, n - 1), min(TILE, n - 1), min(TILE - 1, n - 1)}):   # first, last, last of a wave, tile border
        for b in sorted({0, B - 1}):
            valid = torch.zeros(B, n, dtype=torch.bool)
            valid[b, at] = True
            points, offsets, _, _ = run_and_check(ecm, d, Q, valid.view(B, H, W), 1)
            assert points.shape == (1, 4) and int(points[0, 3]) == b * n + at
            assert offsets.tolist() == [0] * (b + 1) + [1] * (B - b)


@pytest.mark.parametrize("C_", [0, 1, 3, 4])
def test_attribute_counts_and_the_predicate_without_a_valid_plane(ecm, TILE, C_):
    B, H, W = shapes(TILE)["several_tiles"]
    d = disparity(B, H, W, 40 + C_)                                                      # the holes come from the values alone
    run_and_check(ecm, d, matrices(ecm, B, H, W), None, C_, min_disp=20.0, max_disp=150.0)
    run_and_check(ecm, d, matrices(ecm, B, H, W)[1], None, C_, min_disp=0.0, max_disp=INF)   # one shared matrix


def test_bounds_and_zero_w_on_the_device(ecm):
    Q = ecm.ops.q_matrix(100.0, 1.0, 0.5, 0.5)
    d = torch.tensor([[[1.9999999, 2.0, 2.0000002, 7.9999995, 8.0, 8.000001, NAN, INF, -INF, 4.0]]])
    valid = torch.ones(1, 1, 10, dtype=torch.uint8)
    valid[0, 0, 9] = 0
    got = run_and_check(ecm, d, Q, valid, 1, min_disp=2.0, max_disp=8.0)
    assert got[3].cpu().tolist() == [[[False, False, True, True, True, False, False, False, False, False]]]
    run_and_check(ecm, d, Q, valid.bool(), 1, min_disp=2.0 + 2.0 ** -30, max_disp=None)
    zeros = torch.tensor([[[-0.0, 0.0, -0.5, 0.5]]])                                     # W = Q32 d is exactly 0 at the zeros
    points, offsets, xyz, mask = ecm.ops.point_cloud(zeros.to(DEV), Q, None, None, -1.0, None, with_dense=True)
    want = cloud_t(zeros, Q, None, None, -1.0, None)
    assert mask.cpu().tolist() == [[[False, False, True, True]]] and torch.equal(mask.cpu(), want[3])
    assert torch.equal(points.cpu(), want[0]) and offsets.tolist() == [0, 2]
    assert bool((xyz.cpu()[0, :, 0, :2].view(torch.int32) == 0).all())


def test_runs_are_bit_identical_and_a_batch_is_its_images_concatenated(ecm, TILE):
    B, H, W = shapes(TILE)["several_tiles"]
    d, Q = disparity(B, H, W, 77).to(DEV), matrices(ecm, B, H, W)
    valid = pattern("random0.9", B, H, W, TILE).to(DEV)
    colors = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    first = ecm.ops.point_cloud(d, Q, colors, valid, with_dense=True)
    again = ecm.ops.point_cloud(d, Q.to(DEV), colors, valid, with_dense=True)            # Q already on the device, too
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    plain = ecm.ops.point_cloud(d, Q.float(), colors, valid)                             # an fp32 Q is other numbers: the counts only
    assert len(plain) == 2 and plain[1].tolist() == first[1].tolist()
    singles = [ecm.ops.point_cloud(d[i:i + 1], Q[i], colors[i:i + 1], valid[i:i + 1], with_dense=True) for i in range(B)]
    assert torch.equal(torch.cat([s[0] for s in singles]).view(torch.int32), first[0].view(torch.int32))
    assert torch.equal(torch.cat([s[2] for s in singles]).view(torch.int32), first[2].view(torch.int32))
    assert torch.equal(torch.cat([s[3] for s in singles]), first[3])
    assert [int(s[1][1]) for s in singles] == (first[1][1:] - first[1][:-1]).tolist()
    assert torch.equal(ecm.ops.disparity_reproject(d, Q, valid).view(torch.int32), first[2].view(torch.int32))
    assert torch.equal(ecm.ops.disparity_reproject(d.unsqueeze(1), Q, valid.unsqueeze(1)).view(torch.int32), first[2].view(torch.int32))


def test_guard_bands(ecm, TILE):
    """Through the ABI directly, on canary-filled buffers: rows at or beyond N of the worst-case points buffer are untouched, and so
    is a band after xyz, mask, offsets and the scratch buffer."""
    lib = ecm._lib
    B, H, W, C_, BAND, CANARY = 3, 33, 130, 3, 4096, 0xA5
    n = B * H * W
    d = disparity(B, H, W, 13).to(DEV)
    valid = pattern("random0.9", B, H, W, TILE).to(DEV).view(torch.uint8)
    attrs = torch.rand(B, C_, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
    Q = matrices(ecm, B, H, W)
    q = Q.to(DEV)
    nb = int(lib.query("ecmg_point_cloud_scratch_bytes", B, H, W))
    sizes = {"points": n * (3 + C_) * 4, "offsets": (B + 1) * 8, "xyz": n * 12, "mask": n, "scratch": nb}
    bufs = {k: torch.full((v + BAND,), CANARY, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    p = lambda t: C.c_void_p(t.data_ptr())                                               # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.call("ecmg_point_cloud_fwd", p(d), p(valid), p(q), 1, p(attrs), C_, p(bufs["points"]), p(bufs["offsets"]), p(bufs["xyz"]),
             p(bufs["mask"]), p(bufs["scratch"]), C.c_longlong(nb), B, H, W, 0.0, INF, st)
    ecm.ops.check_async_errors()
    want_points, want_offsets, _, want_mask, _ = cloud_t(d.cpu(), Q, attrs.cpu(), valid.cpu())
    N = int(want_offsets[-1])
    assert 0 < N < n
    for k, size in sizes.items():
        assert bool((bufs[k][size:] == CANARY).all()), k
    assert torch.equal(bufs["offsets"][:sizes["offsets"]].view(torch.int64).cpu(), want_offsets)
    rows = bufs["points"][:sizes["points"]].view(torch.float32).view(n, 3 + C_)
    assert bool((bufs["points"][N * (3 + C_) * 4:] == CANARY).all())                     # rows at or beyond N
    assert torch.equal(rows[:N, 3:].cpu(), want_points[:, 3:])
    assert torch.equal(bufs["mask"][:n].view(B, H, W).cpu().bool(), want_mask)
    # the dense entry, the same way
    xyz, mask = (torch.full((s + BAND,), CANARY, dtype=torch.uint8, device=DEV) for s in (n * 12, n))
    lib.call("ecmg_reproject_fwd", p(d), p(valid), p(q), 1, p(xyz), p(mask), B, H, W, 0.0, INF, st)
    ecm.ops.check_async_errors()
    assert bool((xyz[n * 12:] == CANARY).all()) and bool((mask[n:] == CANARY).all())
    assert torch.equal(xyz[:n * 12], bufs["xyz"][:n * 12]) and torch.equal(mask[:n], bufs["mask"][:n])
    # a scratch buffer one byte short is refused before any launch
    with pytest.raises(RuntimeError, match="scratch"):
        lib.call("ecmg_point_cloud_fwd", p(d), p(valid), p(q), 1, p(attrs), C_, p(bufs["points"]), p(bufs["offsets"]), None, None,
                 p(bufs["scratch"]), C.c_longlong(nb - 1), B, H, W, 0.0, INF, st)


def test_runs_on_the_current_stream(ecm, TILE):
    B, H, W = shapes(TILE)["several_tiles"]
    d, Q = disparity(B, H, W, 21), matrices(ecm, B, H, W)
    valid = pattern("random0.9", B, H, W, TILE)
    want = cloud_t(d, Q, None, valid)
    side = torch.cuda.Stream()
    dd, vv = d.to(DEV), valid.to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        points, offsets, xyz, mask = ecm.ops.point_cloud(dd, Q, None, vv, with_dense=True)
        dense = ecm.ops.disparity_reproject(dd, Q, vv)
    side.synchronize()
    ecm.ops.check_async_errors()
    assert torch.equal(offsets.cpu(), want[1]) and torch.equal(mask.cpu(), want[3]) and points.shape == want[0].shape
    assert int(ulps(points.cpu(), want[0]).max()) <= 1 and torch.equal(dense.view(torch.int32), xyz.view(torch.int32))


# ---- what ops.py hands to the second table ----------------------------------------------------------------------------------------------
def test_every_geometry_prototype_is_called_with_well_typed_arguments(ecm, TILE):
    B, H, W = shapes(TILE)["several_tiles"]
    d, Q = disparity(B, H, W, 31).to(DEV), matrices(ecm, B, H, W)
    valid = pattern("random0.9", B, H, W, TILE).to(DEV)
    colors = torch.rand(B, 3, H, W, device=DEV)
    with abi_calls.recording(ecm, "geometry", ecm._lib.GEOMETRY_PROTOTYPES) as calls:
        ecm.ops.point_cloud_tile()
        ecm.ops.disparity_reproject(d, Q, valid, with_mask=True)
        ecm.ops.disparity_reproject(d[:, :, 1:], Q[0].float())                            # a view: made contiguous and aligned
        ecm.ops.point_cloud(d, Q, colors, valid, min_disp=1, max_disp=None, with_dense=True)
        ecm.ops.point_cloud(d.unsqueeze(1), Q, None, None, max_disp=INF)                  # +inf reaches the library as the largest float
        ecm.ops.point_cloud(d, Q, colors.transpose(2, 3).contiguous().transpose(2, 3), valid.view(torch.uint8))
    assert set(calls) == set(ecm._lib.GEOMETRY_PROTOTYPES), sorted(set(ecm._lib.GEOMETRY_PROTOTYPES) - set(calls))
    assert not set(abi_calls.INT_MAX) & set(ecm._lib.GEOMETRY_PROTOTYPES)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
_models = {}


def _model(ecm, arch):
    if arch not in _models:
        torch.manual_seed(5)
        _models[arch] = ecm.get_model(arch).to(DEV).eval()
    return _models[arch]


def _pair(seed=11, hw=256):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(1, 3, hw, hw, device=DEV, generator=gen), torch.randn(1, 3, hw, hw, device=DEV, generator=gen)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def _check_cloud(pc, left, plane, valid):
    assert pc.xyz.shape == (1, 3, 256, 256) and pc.mask.shape == (1, 256, 256) and pc.mask.dtype == torch.bool
    b, y, x = pc.mask.nonzero(as_tuple=True)
    assert torch.equal(pc.points[:, :3].view(torch.int32), pc.xyz[b, :, y, x].view(torch.int32))
    assert torch.equal(pc.points[:, 3:].view(torch.int32), left[b, :, y, x].view(torch.int32))
    assert int(pc.offsets[-1]) == int(pc.mask.sum()) == len(pc.points) and pc.offsets.tolist() == [0, len(pc.points)]
    plane = plane.reshape(1, 256, 256)
    want = torch.isfinite(plane) & (plane > 0)                                            # Q33 = 0: W = d / b, non-zero where d > 0
    if valid is not None:
        want = want & valid.reshape(1, 256, 256)
    assert torch.equal(pc.mask, want)


@pytest.mark.parametrize("arch,source,check", [("cmfsm", "forward", "cross"), ("cmfsm", "smooth", "cross"), ("cmfsm", "smooth", "splat"),
                                               ("cmf", "forward", "cross")])
def test_model_point_cloud(ecm, arch, source, check):
    model, (left, right) = _model(ecm, arch), _pair()
    Q = ecm.ops.q_matrix(721.5, 0.54, 127.3, 131.6)
    with ecm.models.occlusion_check(check), torch.no_grad():
        pc = model.point_cloud(left, right, Q, colors=left, source=source)
        direct = model(left, right) if source == "forward" else getattr(model, source)(left, right)
    assert type(pc.stage) is type(direct) and _same(tuple(pc.stage), tuple(direct))
    plane = direct[2] if source == "forward" else direct.smoothed
    _check_cloud(pc, left, plane, None if source == "forward" else plane > 0)
    assert pc.points.shape[1] == 6
    if source == "forward":
        plain = model.point_cloud(left, right, Q, source="forward")                      # colors=None: XYZ only
        assert plain.points.shape == (len(pc.points), 3) and torch.equal(plain.points.view(torch.int32), pc.points[:, :3].contiguous().view(torch.int32))


def test_the_coordinates_were_within_one_ulp_everywhere():
    """Runs last: how many of the cases above were bit-equal to the restatement (the tolerance stays one ulp either way)."""
    print(f"REPROJECT {EXACT['cases']} cases compared, {EXACT['not_bit_equal']} of them not bit-equal to the fp64 restatement")
    assert EXACT["cases"] > 0
