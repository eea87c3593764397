"""The disparity splat on the MI355X: ops.disparity_splat, _ECMNet.self_check and refine, despeckle and
smooth inside a models.occlusion_check("splat") block against splat_t, the torch fp32 restatement of
tests/test_disp_splat_cpu.py, run on the CPU.

Every comparison is bit for bit -- `right` through .view(torch.int32), `src` as integers.  No tolerance is needed: the only
arithmetic is one fp32 subtraction and a floor, and the reduction is an integer maximum.

Shapes: a single column, fewer columns than a wave, 63/64/65 (a wave of columns), 257 (past the 256-thread stride), 1030 (several
strides), MAX_W (the LDS limit) and 577 rows (more rows than the launch has workgroups, GRID = 512: a workgroup walks on to a
second row and must find its LDS words cleared).  Inputs per shape: general random floats in [0, W/2] and in [-W/4, W/4]; the
contention cases d[x] = x - c, where every pixel of the row lands on column c, from every wave; constant planes (an integral one:
one candidate per column; 2.5: two equal candidates per column, all ties); the step and the ramps of the CPU test; and the first
random case with NaN, +inf and -inf on every 7th column."""
import pytest
import torch

from test_disp_splat_cpu import kernel_constants, ramp_case, splat_t, step_case
from test_hip_guard_bands import POISON, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
KC = kernel_constants()
NAN, INF = float("nan"), float("inf")
SHAPES = [(2, 3, 1), (1, 2, 5), (2, 2, 63), (1, 3, 64), (2, 2, 65), (1, 2, 257), (1, 2, 1030), (1, 1, KC["MAX_W"]), (1, 577, 7)]


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b)


def poison():
    """Fill what the caching allocator will hand out next with NaN (the idea of tests/test_hip_context_fp64.py)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 22,), NAN, device=DEV)] + [torch.full((1 << 14,), NAN, device=DEV) for _ in range(32)]
    del junk


def inputs(shape):
    """name -> d [B,H,W] fp32 on the CPU."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(100 + W + H)
    x = torch.arange(W, dtype=torch.float32).expand(B, H, W)
    out = {"positive": torch.rand(shape, generator=gen) * (W / 2),
           "signed": (torch.rand(shape, generator=gen) - 0.5) * (W / 2)}
    for c in sorted({0, W // 2, W - 1}):
        out[f"all_on_{c}"] = (x - c).contiguous()
    out["constant3"] = torch.full(shape, 3.0)
    out["constant2.5"] = torch.full(shape, 2.5)
    out["step"] = step_case(B, H)[:, :, torch.arange(W) % 256].contiguous()
    out["ramp_up"], out["ramp_down"] = ramp_case(W, 0.3, B, H), ramp_case(W, -0.3, B, H)
    planted = out["positive"].clone()
    for i, v in enumerate((NAN, INF, -INF)):
        planted[:, :, 7 * i::21] = v
    out["planted"] = planted
    return out


def assert_bitwise(ecm, d, what):
    want_right, want_src = splat_t(d)
    right, src = ecm.ops.disparity_splat(d.to(DEV), with_source=True)
    assert right.shape == d.shape and right.dtype == torch.float32 and src.shape == d.shape and src.dtype == torch.int32
    for name, g, r in (("right", bits(right.cpu()), bits(want_right)), ("src", src.cpu().long(), want_src)):
        bad = (g != r).nonzero()
        assert bad.numel() == 0, f"{what}: {name} differs at {bad[:4].tolist()}: {g[tuple(bad[0])]} != {r[tuple(bad[0])]}"
    return right, src


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bit_for_bit(ecm, shape):
    assert KC["MAX_W"] == ecm.ops.disparity_splat_max_width() and 577 > KC["GRID"] and 257 > KC["THREADS"]
    W = shape[2]
    for name, d in inputs(shape).items():
        right, src = assert_bitwise(ecm, d, f"{shape} {name}")
        assert bool(torch.isfinite(right).all())
        if name.startswith("all_on_"):
            c = int(name[7:])                                             # the last column carries the largest disparity
            assert bool((src[:, :, c] == W - 1).all()) and int((src >= 0).sum()) == shape[0] * shape[1]
        if name == "constant2.5" and W >= 4:
            assert bool((src[:, :, 0] == 3).all()) and bool((src[:, :, 1:W - 3] == torch.arange(4, W, device=DEV, dtype=torch.int32)).all())
    ecm.ops.check_async_errors()


def test_source_is_optional_and_the_op_repeats_itself(ecm):
    ops = ecm.ops
    for shape in ((2, 2, 65), (1, 2, 1030), (1, 577, 7)):
        for name in ("positive", "signed", "planted", "constant2.5", "all_on_0"):
            d = inputs(shape)[name].to(DEV)
            right, src = ops.disparity_splat(d, with_source=True)
            alone = ops.disparity_splat(d)
            assert isinstance(alone, torch.Tensor) and same_bits(alone, right)
            poison()
            again, src2 = ops.disparity_splat(d, with_source=True)
            poison()
            assert same_bits(again, right) and torch.equal(src2, src) and same_bits(ops.disparity_splat(d), right)
    ops.check_async_errors()


def test_shapes_strides_and_streams(ecm):
    ops = ecm.ops
    d = inputs((2, 6, 130))["signed"].to(DEV)
    want = ops.disparity_splat(d, with_source=True)
    same = lambda got: same_bits(got[0], want[0]) and torch.equal(got[1], want[1])               # noqa: E731
    assert not want[0].requires_grad and same(ops.disparity_splat(d.unsqueeze(1), with_source=True))
    wide = torch.zeros(2, 6, 260, device=DEV)
    wide[:, :, ::2] = d
    assert not wide[:, :, ::2].is_contiguous() and same(ops.disparity_splat(wide[:, :, ::2], with_source=True))
    assert same(ops.disparity_splat(d.transpose(1, 2).contiguous().transpose(1, 2), with_source=True))
    assert same(ops.disparity_splat(d.clone().requires_grad_(), with_source=True))
    before = d.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.disparity_splat(d, with_source=True)
    side.synchronize()
    assert same(got) and same_bits(d, before)                            # the input is not written
    with pytest.raises(RuntimeError, match="disparity_splat"):
        ops.disparity_splat(d[0, 0])
    with pytest.raises(RuntimeError, match="disparity_splat"):
        ops.disparity_splat(d.view(2, 2, 3, 130))
    with pytest.raises(RuntimeError, match="disparity_splat"):
        ops.disparity_splat(d[:, :0])
    with pytest.raises(RuntimeError, match="fp32"):
        ops.disparity_splat(d.double())
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_splat(d.cpu())
    ops.check_async_errors()


def test_guard_bands_and_the_width_refusal(ecm):
    ops = ecm.ops
    for shape in SHAPES:
        d = inputs(shape)["signed"].to(DEV)
        with guarded(ecm) as g:
            ops.disparity_splat(d, with_source=True)
            g.check(f"disparity_splat {shape}")
            assert len(g.records) == 2                               # right, src
        with guarded(ecm) as g:
            ops.disparity_splat(d)
            g.check(f"disparity_splat {shape} without src")
            assert len(g.records) == 1
    wide = torch.zeros(1, 2, ops.disparity_splat_max_width() + 1, device=DEV)
    with guarded(ecm) as g:
        with pytest.raises(RuntimeError, match="not supported"):
            ops.disparity_splat(wide, with_source=True)
        g.check("disparity_splat beyond the maximum width")
        assert len(g.records) == 2
        for raw, off, n in g.records:
            assert bool((raw[off:off + n] == POISON).all()), "a refused call wrote to its outputs"
    ops.check_async_errors()


def test_the_check_of_a_splat_on_the_device(ecm):
    """ops.lr_check of a map against its own splat: the closed forms of the CPU test, from the two kernels."""
    ops = ecm.ops
    d = step_case(2, 3).to(DEV)
    error, kind, _ = ops.lr_check(d, ops.disparity_splat(d), 1.0, 0.0)
    assert bool(((kind == 1).sum(2) == 26).all()) and not bool((kind == 2).any()) and bool((kind[:, :, 74:100] == 1).all())
    for name in ("positive", "signed", "ramp_up", "ramp_down", "planted"):
        d = inputs((2, 2, 1030))[name].to(DEV)
        error, kind, _ = ops.lr_check(d, ops.disparity_splat(d), 1.0, 0.0)
        assert bool(((kind == 0) | (kind == 1) | (kind == 3)).all()), name
        assert bool((error >= 0).all()) and torch.equal(torch.isfinite(error), kind != 3), name
        if name.startswith("ramp"):
            assert bool((kind[kind != 3] == 0).all())
    ops.check_async_errors()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
FRAMES = {"cmfsm": (256, 256), "cmfsm_sub_8": (256, 256), "cmf": (256, 512)}     # the small frames of the post-filter suites; cmf's own


@pytest.fixture(scope="module", params=["cmfsm", "cmfsm_sub_8", "cmf"])
def net(request, ecm):
    H, W = FRAMES[request.param]
    torch.manual_seed(5)
    model = ecm.get_model(request.param).to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    left, right = torch.randn(1, 3, H, W, device=DEV, generator=gen), torch.randn(1, 3, H, W, device=DEV, generator=gen)
    return model, left, right


def test_self_check(ecm, net):
    ops = ecm.ops
    model, left, right = net
    H, W = left.shape[-2:]
    kw = dict(threshold=1.0, rel=0.05)
    with torch.no_grad():
        heads = [p.reshape(1, 1, H, W) for p in model(left, right)]
    sc = model.self_check(left, right, **kw)
    assert type(sc).__name__ == "CrossCheck" and all(f.shape == (1, 1, H, W) and not f.requires_grad for f in sc)
    assert same_bits(sc.disparity, heads[2]), ".disparity differs from forward"
    assert same_bits(sc.disparity_right[:, 0], ops.disparity_splat(sc.disparity))
    again = ops.lr_check(sc.disparity, sc.disparity_right, 1.0, 0.05, mirrored=False)
    assert all(same_bits(f[:, 0], a) for f, a in zip(sc[2:], again))
    assert not bool((sc.kind == 2).any()) and bool((sc.error >= 0).all())
    assert same_bits(model.self_check(left, right, head=0).disparity, heads[0])
    # the restatement on the net's own disparity
    want_right, _ = splat_t(sc.disparity[:, 0].cpu())
    assert torch.equal(bits(sc.disparity_right[:, 0].cpu()), bits(want_right))
    ops.check_async_errors()


def test_the_chains_on_a_splat(ecm, net):
    ops, splat = ecm.ops, ecm.models.occlusion_check("splat")
    model, left, right = net
    kw = dict(threshold=1.0, rel=0.05)
    sc = model.self_check(left, right, **kw)
    with splat:
        smoothed = model.smooth(left, right, speckle_size=50, speckle_diff=0.5, lam=512.0, sigma_color=1.5, iterations=2, **kw)
        refined = model.refine(left, right, median_radius=1, bilateral_radius=2, **kw)
        despeckled = model.despeckle(left, right, median_radius=1, bilateral_radius=2, speckle_size=50, speckle_diff=0.5, **kw)
        inside = model.cross_check(left, right, **kw), model.self_check(left, right, **kw)
    # smooth
    out = smoothed
    assert type(out).__name__ == "Smoothed" and all(same_bits(a, b) for a, b in zip(out[:5], sc))
    _, _, size = ops.disparity_speckle(sc.disparity, sc.kind == 0, 50, 0.5, with_segments=True)
    confidence = ((sc.kind[:, 0] == 0) & (size > 50)).float()
    assert torch.equal(out.confidence[:, 0], confidence)
    assert same_bits(out.smoothed[:, 0], ops.disparity_wls(sc.disparity, left, confidence, 512.0, 1.5, 2))
    # refine
    out = refined
    assert type(out).__name__ == "Refined" and all(same_bits(a, b) for a, b in zip(out[:5], sc))
    median = ops.disparity_median(sc.filled, sc.filled > 0, 1).unsqueeze(1)
    assert same_bits(out.median, median)
    assert same_bits(out.refined[:, 0], ops.disparity_bilateral(median, left, median > 0, 2, 2.0, 0.25))
    # despeckle
    out = despeckled
    assert type(out).__name__ == "Despeckled" and all(same_bits(a, b) for a, b in zip(out[:5], sc))
    kept, _, size = ops.disparity_speckle(sc.disparity, sc.kind == 0, 50, 0.5, with_segments=True)
    _, kind, filled, src = ops.lr_check(sc.disparity, sc.disparity_right, 1.0, 0.05, with_source=True)
    take = (src >= 0) & (torch.gather(kept, 2, src.clamp(min=0).long()) > 0)
    despeckled = torch.where(take, filled, torch.zeros_like(filled)).unsqueeze(1)
    assert torch.equal(out.segment[:, 0], size) and same_bits(out.despeckled, despeckled)
    median = ops.disparity_median(despeckled, despeckled > 0, 1).unsqueeze(1)
    assert same_bits(out.median, median)
    assert same_bits(out.refined[:, 0], ops.disparity_bilateral(median, left, median > 0, 2, 2.0, 0.25))
    # cross_check and self_check do not look at the block
    assert all(same_bits(a, b) for a, b in zip(inside[0], model.cross_check(left, right, **kw)))
    assert all(same_bits(a, b) for a, b in zip(inside[1], sc)) and not same_bits(inside[0].disparity_right, sc.disparity_right)
    ops.check_async_errors()


def test_cross_is_the_call_outside_the_block(ecm, net):
    model, left, right = net
    kw = dict(threshold=1.0, rel=0.05)
    for method, more in ((model.smooth, dict(speckle_size=50, iterations=2)), (model.refine, dict(median_radius=1, bilateral_radius=2)),
                         (model.despeckle, dict(median_radius=1, bilateral_radius=2, speckle_size=50))):
        plain = method(left, right, **kw, **more)
        with ecm.models.occlusion_check("cross"):
            cross = method(left, right, **kw, **more)
        with ecm.models.occlusion_check("splat"):
            pass
        after = method(left, right, **kw, **more)                        # the block restores the default
        assert type(plain) is type(cross) is type(after), method.__name__
        assert all(same_bits(a, b) and same_bits(a, c) for a, b, c in zip(plain, cross, after)), method.__name__
    cc = model.cross_check(left, right, **kw)
    assert all(same_bits(a, b) for a, b in zip(plain[:5], cc))
    with pytest.raises(ValueError, match="check"):
        with ecm.models.occlusion_check("both"):
            model.smooth(left, right)
    ecm.ops.check_async_errors()
