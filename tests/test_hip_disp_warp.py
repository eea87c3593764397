"""ops.disparity_warp, ops.disparity_fuse and models.DisparityTracker on the MI355X against warp_t and
fuse_t of tests/test_disp_warp_cpu.py, run on the CPU.

The warp is compared bit for bit -- `out` and `attrs_out` through .view(torch.int32), `src` as integers -- under both footprints.
No tolerance is needed: the device evaluates the same IEEE fp64 expressions in the same order without fused multiply-adds, the
divisions are true divisions, and the reduction is an integer maximum.  Shapes: a single column, fewer columns than a wave,
63/64/65 columns at 5 rows, 257 x 130 (17 tiles, the last partial, rows that straddle tiles), 33 x 577, a [3,40,70] batch with a
matrix per image, and 256 x 256 for the contention case (65536 candidates on one address).

The fusion's decisions (branch, age) are exact against fuse_t: the inputs are constructed so that the gate's two sides are at
least 1e-3 (relative) apart, which the draw asserts for every pixel; copied outputs are compared bit for bit; `fused` is within
4 * 2^-23 * max(|disp|, |prev|) and `fused_var` within 4 * 2^-23 * s of the fp64 restatement (at most eight rounded fp32
operations of relative error 2^-24 each lie between the inputs and either output)."""
import ctypes as C

import pytest
import torch

from test_disp_warp_cpu import BRANCHES, FOOTPRINTS, axial, bits, fuse_t, quantised, rigid, shear, warp_t
from test_hip_guard_bands import POISON, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
SHAPES = [(2, 3, 1), (1, 2, 5), (1, 5, 63), (1, 5, 64), (1, 5, 65), (1, 257, 130), (1, 33, 577), (3, 40, 70)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def poison():
    """Fill what the caching allocator will hand out next with NaN (the idea of tests/test_hip_context_fp64.py)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 22,), NAN, device=DEV)] + [torch.full((1 << 14,), NAN, device=DEV) for _ in range(32)]
    del junk


def rigid_matrix(ecm, B, H, W):
    """M = Q^-1 T Q of a small rotation plus a translation (mostly forward); one per image for B >= 3, else shared."""
    ops = ecm.ops
    Q = ops.q_matrix(0.9 * max(W, H) + 3.3, 0.5, 0.47 * W + 0.123, 0.45 * H + 0.217)
    T = rigid(0.004, -0.006, 0.01, 0.03, -0.02, -0.4)
    if B < 3:
        return ops.warp_matrix(Q, T)
    Ts = torch.stack([T, rigid(-0.01, 0.003, -0.02, -0.05, 0.01, 0.3), torch.eye(4, dtype=torch.float64)] + [T] * (B - 3))
    return ops.warp_matrix(Q, Ts)


def disparity(B, H, W, seed, holes=True):
    g = torch.Generator().manual_seed(seed)
    d = 0.5 + (0.25 * W + 8.0) * torch.rand(B, H, W, generator=g)
    if holes:
        r = torch.rand(B, H, W, generator=g)
        for k, bad in enumerate((NAN, INF, -INF, 0.0, -0.0, -3.5)):
            d[(r >= 0.02 * k) & (r < 0.02 * (k + 1))] = bad
    return d


def one_site(cx, cy):
    """Rows 0 and 1 constant: every usable pixel lands about (cx, cy) with its own disparity."""
    M = torch.eye(4, dtype=torch.float64)
    M[0], M[1] = torch.tensor([0, 0, 0, cx], dtype=torch.float64), torch.tensor([0, 0, 0, cy], dtype=torch.float64)
    return M


def attributes(B, Cn, H, W):
    """Plane 0 is the pixel's index within the batch (< 2^24: exact in fp32), the rest random."""
    if Cn is None:
        return None
    index = torch.arange(B * H * W, dtype=torch.float32).view(B, 1, H, W)
    extra = torch.rand(B, max(Cn - 1, 0), H, W, generator=torch.Generator().manual_seed(Cn))
    return torch.cat([index, extra], 1)[:, :Cn].contiguous()


def dev(t):
    return None if t is None else t.to(DEV)


def call(ecm, d, M, valid, attrs, footprint, **kw):
    """(out, src, attrs_out) of ops.disparity_warp on the device, whatever the combination of outputs."""
    got = ecm.ops.disparity_warp(dev(d), M, dev(valid), dev(attrs), footprint=footprint, with_source=True, **kw)
    return (got[0], got[-1], got[1] if attrs is not None else None)


def assert_bitwise(ecm, d, M, valid, attrs, footprint, what, **kw):
    want_out, want_src, want_attrs = warp_t(d, M, valid, attrs, footprint=footprint, **kw)
    out, src, attrs_out = call(ecm, d, M, valid, attrs, footprint, **kw)
    B, H, W = d.shape
    assert out.shape == (B, 1, H, W) and out.dtype == torch.float32 and src.shape == (B, 1, H, W) and src.dtype == torch.int32
    pairs = [("out", bits(out.cpu()[:, 0]), bits(want_out)), ("src", src.cpu()[:, 0].long(), want_src)]
    if attrs is not None:
        assert attrs_out.shape == attrs.shape and attrs_out.dtype == torch.float32
        pairs.append(("attrs_out", bits(attrs_out.cpu()), bits(want_attrs)))
    for name, g, r in pairs:
        bad = (g != r).nonzero()
        assert bad.numel() == 0, f"{what}: {name} differs at {bad[:4].tolist()}: {g[tuple(bad[0])]} != {r[tuple(bad[0])]}"
    return out, src, attrs_out


def same(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and torch.equal(bits(x) if x.dtype == torch.float32 else x,
                                                                                bits(y) if y.dtype == torch.float32 else y))
               for x, y in zip(a, b))


# ---- the warp, bit for bit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("footprint", FOOTPRINTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bit_for_bit(ecm, shape, footprint):
    B, H, W = shape
    M = rigid_matrix(ecm, B, H, W)
    g = torch.Generator().manual_seed(H + W)
    valid = torch.rand(B, H, W, generator=g) < 0.9
    planted, clean = disparity(B, H, W, 7 * H + W), disparity(B, H, W, 3 * H + W, holes=False)
    cases = [("rigid, planted non-finite values, bool valid, C = 4", planted, M, valid, attributes(B, 4, H, W)),
             ("rigid, uint8 valid, C = 1", clean, M, valid.to(torch.uint8) * 3, attributes(B, 1, H, W)),
             ("rigid, C = 0", clean, M, None, None),
             ("identity", planted, torch.eye(4, dtype=torch.float64), None, attributes(B, 1, H, W)),
             ("shear", quantised(B, H, W, 11), shear(), None, None),
             ("forward motion", clean, axial(1.0 / (16.0 * (0.25 * W + 9.0))), None, attributes(B, 1, H, W)),
             ("every pixel onto one site", clean, one_site(W // 2, H // 2), None, attributes(B, 1, H, W)),
             ("every pixel onto four sites", planted, one_site(0.5 * (W - 1) * 0.999, 0.5 * (H - 1) * 0.999), valid, None)]
    hit = 0
    for name, d, m, v, a in cases:
        out, src, _ = assert_bitwise(ecm, d, m, v, a, footprint, f"{shape} {footprint} {name}")
        hit += int((src >= 0).sum())
        if name == "identity":
            usable = torch.isfinite(d) & (d > 0)
            assert torch.equal(bits(out.cpu()[:, 0]), torch.where(usable, bits(d), 0))
        if name == "every pixel onto one site":                            # the winner is the largest key: disparity, then index
            for b in range(B):
                top = d[b].flatten().max()
                last = int((d[b].flatten() == top).nonzero().max())
                assert int((src[b] >= 0).sum()) == 1 and int(src[b, 0, H // 2, W // 2]) == last
                assert bits(out[b, 0, H // 2, W // 2].cpu()) == bits(top)
    assert hit > 0
    # again on what a NaN-filled allocator hands out, and on a side stream: the same bits
    name, d, m, v, a = cases[0]
    first = call(ecm, d, m, v, a, footprint)
    poison()
    again = call(ecm, d, m, v, a, footprint)
    poison()
    side = torch.cuda.Stream()
    operands = [dev(d), dev(v), dev(a)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        third = ecm.ops.disparity_warp(operands[0], m, operands[1], operands[2], footprint=footprint, with_source=True)
    side.synchronize()
    assert same(first, again) and same(first, (third[0], third[2], third[1]))
    ecm.ops.check_async_errors()


@pytest.mark.parametrize("footprint", FOOTPRINTS)
def test_sixty_four_thousand_candidates_on_one_address(ecm, footprint):
    B, H, W = 1, 256, 256
    d = disparity(B, H, W, 5, holes=False)
    d[0, 100, 17], d[0, 200, 33] = 500.0, 500.0                            # the largest disparity twice: the larger index wins
    out, src, attrs = assert_bitwise(ecm, d, one_site(3, 250), None, attributes(B, 2, H, W), footprint, "one site")
    assert int((src >= 0).sum()) == 1 and int(src[0, 0, 250, 3]) == 200 * W + 33 and float(out[0, 0, 250, 3]) == 500.0
    assert float(attrs[0, 0, 250, 3]) == 200 * W + 33
    ecm.ops.check_async_errors()


def test_the_shear_is_the_splat_kernel(ecm):
    """M = I with M[0][2] = -1 against ops.disparity_splat itself, on the 1/64 px grid where the splat's fp32 x - d is exact."""
    for B, H, W in ((2, 5, 65), (1, 33, 577), (3, 40, 70)):
        d = quantised(B, H, W, H + W).to(DEV)
        right, col = ecm.ops.disparity_splat(d, with_source=True)
        out, src = ecm.ops.disparity_warp(d, shear(), with_source=True)
        rows = (torch.arange(H, device=DEV, dtype=torch.int32) * W).view(1, H, 1)
        assert torch.equal(bits(out[:, 0]), bits(right))
        assert torch.equal(torch.where(src[:, 0] >= 0, src[:, 0] - rows, -1), col)
    ecm.ops.check_async_errors()


def test_return_forms_strides_and_a_batch_is_its_images(ecm):
    ops = ecm.ops
    B, H, W = 3, 40, 70
    M = rigid_matrix(ecm, B, H, W)
    d, a = disparity(B, H, W, 3).to(DEV), attributes(B, 4, H, W).to(DEV)
    valid = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(1)) < 0.9).to(DEV)
    out, attrs_out, src = ops.disparity_warp(d, M, valid, a, with_source=True)
    alone = ops.disparity_warp(d, M, valid)
    assert isinstance(alone, torch.Tensor) and torch.equal(bits(alone), bits(out)) and not out.requires_grad
    pair = ops.disparity_warp(d, M, valid, with_source=True)
    assert len(pair) == 2 and torch.equal(pair[1], src)
    pair = ops.disparity_warp(d, M, valid, a)
    assert len(pair) == 2 and torch.equal(bits(pair[1]), bits(attrs_out))
    empty = ops.disparity_warp(d, M, valid, a[:, :0])
    assert len(empty) == 2 and empty[1].shape == (B, 0, H, W) and torch.equal(bits(empty[0]), bits(out))
    want = (out, attrs_out, src)
    # [B,1,H,W] planes, a matrix already on the device, strided operands (served as the sibling ops serve them: made contiguous)
    assert same(ops.disparity_warp(d.unsqueeze(1), M.to(DEV), valid.unsqueeze(1), a, with_source=True), want)
    wide = torch.zeros(B, H, 2 * W, device=DEV)
    wide[:, :, ::2] = d
    strided_a = a.transpose(2, 3).contiguous().transpose(2, 3)
    assert not wide[:, :, ::2].is_contiguous() and not strided_a.is_contiguous()
    assert same(ops.disparity_warp(wide[:, :, ::2], M, valid.view(torch.uint8), strided_a, with_source=True), want)
    before = d.clone()
    singles = [ops.disparity_warp(d[i:i + 1], M[i], valid[i:i + 1], a[i:i + 1], with_source=True) for i in range(B)]
    for k in range(3):
        assert torch.equal(torch.cat([s[k] for s in singles]).view(torch.int32), want[k].view(torch.int32))
    assert torch.equal(bits(d), bits(before))                              # the input is not written
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_warp(d.cpu(), M)
    with pytest.raises(ValueError, match="one matrix, or one per image"):
        ops.disparity_warp(d[:2], M)
    ops.check_async_errors()


def test_guard_bands_and_the_short_scratch(ecm):
    ops, lib = ecm.ops, ecm._lib
    for shape in SHAPES:
        B, H, W = shape
        d, M, a = disparity(B, H, W, 13).to(DEV), rigid_matrix(ecm, B, H, W), attributes(B, 4, H, W).to(DEV)
        for footprint in FOOTPRINTS:
            with guarded(ecm) as g:
                ops.disparity_warp(d, M, None, a, footprint=footprint, with_source=True)
                g.check(f"disparity_warp {shape} {footprint}")
                assert len(g.records) == 4                                 # out, src, attrs_out, the keys
        with guarded(ecm) as g:
            ops.disparity_warp(d, one_site(W - 1, H - 1))                  # everything onto the last pixel of each image
            g.check(f"disparity_warp {shape} onto the last site")
            assert len(g.records) == 2
        with guarded(ecm) as g:
            z = torch.rand(B, H, W, device=DEV) + 0.5
            ops.disparity_fuse(z, z, z, z, None, z)
            g.check(f"disparity_fuse {shape}")
            assert len(g.records) == 3
    # one byte short of the query: refused before any launch, the outputs untouched
    B, H, W = 3, 40, 70
    n = B * H * W
    d, m = disparity(B, H, W, 13).to(DEV), rigid_matrix(ecm, B, H, W).to(DEV)
    nb = int(lib.query("ecmt_disparity_warp_scratch_bytes", B, H, W))
    assert nb == 8 * n
    out, src, keys = (torch.full((s,), POISON, dtype=torch.uint8, device=DEV) for s in (4 * n, 4 * n, nb))
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="scratch"):
        lib.call("ecmt_disparity_warp_fwd", p(d), None, p(m), 1, None, 0, p(out), p(src), None, p(keys), C.c_longlong(nb - 1),
                 B, H, W, 0.0, INF, 0, st)
    torch.cuda.synchronize()
    assert all(bool((t == POISON).all()) for t in (out, src, keys))
    lib.call("ecmt_disparity_warp_fwd", p(d), None, p(m), 1, None, 0, p(out), p(src), None, p(keys), C.c_longlong(nb),
             B, H, W, 0.0, INF, 0, st)
    want = ops.disparity_warp(d, m, with_source=True)
    assert torch.equal(out.view(torch.int32), want[0].view(torch.int32).flatten()) and torch.equal(src.view(torch.int32), want[1].flatten())
    ops.check_async_errors()


# ---- the fusion --------------------------------------------------------------------------------------------------------------------------
def fusion_inputs(shape, seed, gate, noise, with_source):
    """Planes whose gate decisions cannot depend on fp32 rounding: where both a measurement and a prediction exist, disp is
    placed at prev +- sqrt(rho gate^2 (s + var)) with rho in [0, 0.9] or [1.1, 4]; then the other four combinations are planted."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda: torch.rand(shape, generator=g, dtype=torch.float64)                           # noqa: E731
    prev = (20.0 + 80.0 * rand()).float()
    pvar = (0.05 + 1.95 * rand()).float()
    var = (0.05 + 1.95 * rand()).float()
    source = (prev.double() * (0.8 + 0.45 * rand())).float() if with_source else None
    page = torch.randint(0, 1000, shape, generator=g, dtype=torch.int32)
    _, _, _, _, s, _ = fuse_t(prev, var, prev, pvar, page, source, gate, noise)
    rho = torch.where(rand() < 0.5, 0.9 * rand(), 1.1 + 2.9 * rand())
    sign = torch.where(rand() < 0.5, -1.0, 1.0)
    g32 = float(torch.tensor(gate, dtype=torch.float32))
    disp = (prev.double() + sign * torch.sqrt(rho * g32 * g32 * (s + var.double()))).float()
    assert bool((disp > 0).all())
    r = rand()
    for k, bad in enumerate((NAN, 0.0, -2.0, INF)):                        # no measurement
        disp[(r >= 0.03 * k) & (r < 0.03 * (k + 1))] = bad
    for k, bad in enumerate((0.0, NAN, -1.0, INF)):
        var[(r >= 0.12 + 0.02 * k) & (r < 0.12 + 0.02 * (k + 1))] = bad
    r = rand()
    for k, bad in enumerate((0.0, -0.0, NAN, -5.0)):                       # no prediction
        prev[(r >= 0.03 * k) & (r < 0.03 * (k + 1))] = bad
    for k, bad in enumerate((0.0, NAN, -1.0, INF)):
        pvar[(r >= 0.12 + 0.02 * k) & (r < 0.12 + 0.02 * (k + 1))] = bad
    margin = fuse_t(disp, var, prev, pvar, page, source, gate, noise)[5]
    assert bool((margin > 1e-3).all()), float(margin.min())               # every pixel: no case is left out
    return disp, var, prev, pvar, page, source


@pytest.mark.parametrize("with_source", [False, True], ids=["plain", "axial"])
@pytest.mark.parametrize("coast", [True, False], ids=["coast", "drop"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 37, 130), (1, 257, 1030)], ids=["1x1x1", "2x37x130", "1x257x1030"])
def test_fusion_decisions_are_exact_and_values_within_four_ulps(ecm, shape, coast, with_source):
    gate, noise = (3.0, 0.01) if coast else (1.5, 0.0)
    disp, var, prev, pvar, page, source = fusion_inputs(shape, sum(shape) + coast, gate, noise, with_source)
    want_f, want_v, want_age, branch, s, _ = fuse_t(disp, var, prev, pvar, page, source, gate, noise, coast)
    if shape[1] > 1:
        assert sorted(set(branch.flatten().tolist())) == [0, 1 if coast else 2, 3, 4, 5]       # every branch occurs
    fused, fvar, age = (t.cpu()[:, 0] for t in ecm.ops.disparity_fuse(dev(disp), dev(var), dev(prev), dev(pvar), dev(page),
                                                                        dev(source), gate, noise, coast))
    assert fused.dtype == fvar.dtype == torch.float32 and age.dtype == torch.int32
    assert torch.equal(age.long(), want_age)
    zero = lambda t, m: bool((bits(t)[m] == 0).all())                                            # noqa: E731
    for b in (0, 2):                                                       # neither, dropped: +0.0
        assert zero(fused, branch == b) and zero(fvar, branch == b)
    copied = (branch == 3) | (branch == 4)                                 # the measurement, bit for bit
    assert torch.equal(bits(fused)[copied], bits(disp)[copied]) and torch.equal(bits(fvar)[copied], bits(var)[copied])
    assert torch.equal(bits(fused)[branch == 1], bits(prev)[branch == 1])  # coasting: the prediction, bit for bit
    live = (branch == 1) | (branch == 5)
    tol_f = 4 * 2.0 ** -23 * torch.maximum(disp.double().abs(), prev.double().abs())
    tol_v = 4 * 2.0 ** -23 * s
    err_f, err_v = (fused.double() - want_f).abs(), (fvar.double() - want_v).abs()
    both = branch == 5                                                     # a coasting `fused` is held bit for bit above; its disp may be NaN
    if bool(both.any()):
        print(f"FUSE {shape} {BRANCHES[1 if coast else 2]} source={with_source}: worst fused error "
              f"{float((err_f / tol_f)[both].max()):.3f}, worst variance error {float((err_v / tol_v)[live].max()):.3f} of the bound")
    assert bool((err_f[both] <= tol_f[both]).all()) and bool((err_v[live] <= tol_v[live]).all())
    # without prev_age the ages count from zero
    fused2, fvar2, age2 = ecm.ops.disparity_fuse(dev(disp), dev(var), dev(prev), dev(pvar), None, dev(source), gate, noise, coast)
    assert torch.equal(bits(fused2.cpu()[:, 0]), bits(fused)) and torch.equal(bits(fvar2.cpu()[:, 0]), bits(fvar))
    assert torch.equal(age2.cpu()[:, 0].long(), torch.where(branch >= 3, 1, 0))
    ecm.ops.check_async_errors()


# ---- the tracker -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,hw", [("cmfsm", (256, 512)), ("cmfsm_sub_8", (256, 256))])
def test_tracker_is_the_ops_assembled_by_hand(ecm, arch, hw):
    ops, models = ecm.ops, ecm.models
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    frames = [(torch.randn(1, 3, *hw, device=DEV, generator=gen), torch.randn(1, 3, *hw, device=DEV, generator=gen)) for _ in range(2)]
    Q = ops.q_matrix(700.0, 0.25, 0.5 * hw[1], 0.5 * hw[0])
    motion = rigid(0.002, -0.003, 0.001, 0.01, 0.0, -0.05)
    gate, noise, sigma0 = 3.0, 0.01, 1.5
    tracker = models.DisparityTracker(model, Q, gate=gate, process_noise=noise, sigma0=sigma0)
    same_bits = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))   # noqa: E731

    def own(left, right):
        with torch.no_grad():
            disparity = model(left, right)[2].reshape(1, 1, *hw)
        if arch == "cmfsm":
            std = model.predict(left, right, (2,)).std[0]
        else:
            std = torch.full_like(disparity, sigma0)
        return disparity, std

    def started_over(t, left, right):
        disparity, std = own(left, right)
        zeros = torch.zeros_like(disparity)
        hand = ops.disparity_fuse(disparity, std * std, zeros, zeros, zeros.to(torch.int32), zeros, gate, noise, True)
        assert isinstance(t, models.Tracked) and all(f.shape == (1, 1, *hw) for f in t)
        assert same_bits(t.disparity, disparity) and same_bits(t.std, std) and bool((t.warped.view(torch.int32) == 0).all())
        assert same_bits(t.fused, hand[0]) and same_bits(t.variance, hand[1]) and torch.equal(t.age, hand[2])
        assert t.age.dtype == torch.int32 and int(t.age.max()) <= 1

    first = tracker(*frames[0], motion=motion)                             # a first frame starts over whatever the motion
    started_over(first, *frames[0])
    second = tracker(*frames[1], motion=motion)
    disparity, std = own(*frames[1])
    M = ops.warp_matrix(Q, motion)
    carried_in = torch.cat([first.variance, first.fused, first.age.to(torch.float32)], 1)
    warped, carried = ops.disparity_warp(first.fused, M, attributes=carried_in)
    hand = ops.disparity_fuse(disparity, std * std, warped, carried[:, 0:1], carried[:, 2:3].to(torch.int32), carried[:, 1:2],
                              gate, noise, True)
    assert same_bits(second.disparity, disparity) and same_bits(second.std, std) and same_bits(second.warped, warped)
    assert same_bits(second.fused, hand[0]) and same_bits(second.variance, hand[1]) and torch.equal(second.age, hand[2])
    # the comparison is not vacuous: part of the state arrives (with untrained weights the heads are not bounded, so much of it
    # may leave the view)
    assert int((warped > 0).sum()) > 1000 and int(second.age.max()) <= 2
    started_over(tracker(*frames[0]), *frames[0])                          # motion=None
    tracker(*frames[1], motion=motion)
    tracker.reset()
    started_over(tracker(*frames[1], motion=motion), *frames[1])           # reset()
    pair = tuple(torch.cat([f, f]) for f in frames[0])                     # a changed shape
    assert bool((tracker(*pair, motion=motion).warped == 0).all())
    ops.check_async_errors()
