"""color.volume_integrate, color.volume_raycast, color.volume_sample, color.mesh_colors and models.ColorStereoMapper on the MI355X
 against integrate_color_t, raycast_color_t and sample_t of tests/test_volume_color_cpu.py, run on the CPU,
and against ops.volume_integrate and ops.volume_raycast on the device, whose results they must leave bit for bit.

The per-voxel, per-pixel and per-point arithmetic of the device is the restatement's, operation for operation (IEEE fp64 and fp32
without fused multiply-adds), so bit-equality is expected; one ulp of fp32 is allowed, and every test prints the largest
difference it saw.  Holes must be equal as sets.  The volumes and images are those of tests/test_hip_disp_volume.py: 1x1x1,
3x5x7, one brick of the 16-byte path exactly (4x4x64), the 4-byte path plus one (5x5x17, 5x5x65), a partial brick of the 16-byte
path (4x4x16), one brick plus one thread (9x6x68); and one volume with nx % 4 == 0 whose attr starts one float off alignment."""
import pytest
import torch

from test_disp_volume_cpu import (DIMS, F32, F64, FAR, FIFTH, H0, HIT_SHARE, MAPPER_HELD_OUT, MAPPER_MIN_DISP, MAPPER_STD, NEAR, ORIGIN, TRUNC, VIEWS, VOXEL, W0,
                                  mapper_maps, mapper_poses, scene_views)
from test_disp_warp_cpu import bits, rigid
from test_hip_disp_volume import POSES, box, ulps, used_volume, views
from test_hip_guard_bands import guarded
from test_motion_align_cpu import scene_q
from test_volume_color_cpu import (COLOR_BOUND, MAPPER_COLOR_BOUND, MAPPER_VERTEX_COLOR_BOUND, VERTEX_COLOR_BOUND, affine_colors, color_error, color_loop, dirty_attributes, integrate_color_t,
                                   raycast_color_t, sample_t, scene_colors, used_attributes, world_points)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def dev(t):
    return None if t is None else t.to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


# ---- integrate --------------------------------------------------------------------------------------------------------------------------
# (dims, image, V, per-view matrices, valid and weight planes, A)
CASES = [((1, 1, 1), (2, 2), 1, False, False, 1), ((3, 5, 7), (37, 61), 3, True, True, 3), ((4, 4, 64), (40, 64), 1, False, True, 4),
         ((5, 5, 65), (40, 64), 3, False, False, 3), ((4, 4, 16), (37, 61), 3, True, False, 1), ((5, 5, 17), (40, 64), 1, False, True, 4),
         ((9, 6, 68), (40, 64), 3, True, True, 3), ((9, 6, 68), (37, 61), 3, False, True, 4), ((4, 4, 64), (2, 2), 3, True, False, 1),
         ((6, 7, 12), (40, 64), 1, True, True, 3)]
KW = lambda W: dict(max_weight=2.5, min_disp=0.05, max_disp=1.25 * W * 0.25 / 2.7)              # noqa: E731  (nearer than 2.7 m is gated out)


def run_integrate(ecm, case, offset=0):
    """One case on the device and in the restatement; offset: attr starts that many floats into its allocation."""
    ops, color = ecm.ops, ecm.color
    dims, (H, W), V, per_view, planes, A = case
    origin, voxel = box(dims)
    d, Q, (valid, w) = views(V, H, W, 7 * H + W + V, planes)
    c = dirty_attributes(V, A, H, W, 3 * H + A)
    T = torch.stack(POSES[:V]) if per_view else POSES[0]
    kw = KW(W)
    tsdf0, wsum0 = used_volume(dims, sum(dims))
    attr0, asum0 = used_attributes(dims, A, sum(dims) + 1)
    m = ops.volume_matrices(Q, T, origin, voxel)
    want = integrate_color_t(tsdf0, wsum0, attr0, asum0, d, c, Q, m.G, m.C, TRUNC, valid, w, **kw)

    def start():
        raw = torch.zeros(attr0.numel() + offset, device=DEV)
        attr = raw[offset:].view(attr0.shape)
        attr.copy_(attr0)
        return tsdf0.to(DEV), wsum0.to(DEV), attr, asum0.to(DEV)

    vol = start()
    if offset:
        assert vol[2].data_ptr() % 16 == 4 * offset and vol[0].data_ptr() % 16 == 0 and dims[2] % 4 == 0
    back = color.volume_integrate(*vol, d.to(DEV), c.to(DEV), Q, T, origin, voxel, TRUNC, dev(valid), dev(w), **kw)
    assert all(b is v for b, v in zip(back, vol))                          # in place
    got = [t.cpu() for t in vol]
    seen = tuple(ulps(g, x) for g, x in zip(got, want[:4]))
    touched, coloured = want[4], want[5]
    print("integrate", case, "offset", offset, "touched", int(touched.sum()), "coloured", int(coloured.sum()), "of", touched.numel(),
          "ulps (tsdf, wsum, attr, asum)", seen)
    assert max(seen) <= 1, seen
    assert not bool(torch.isnan(got[2]).any()) and not bool(torch.isinf(got[2]).any())           # no NaN or Inf of the images got in
    assert torch.equal(bits(got[2])[:, ~coloured], bits(attr0)[:, ~coloured]) and torch.equal(bits(got[3])[~coloured], bits(asum0)[~coloured])
    # tsdf and wsum are ops.volume_integrate's on the device: bit equality, no ulp
    plain = ops.volume_integrate(tsdf0.to(DEV), wsum0.to(DEV), d.to(DEV), Q, T, origin, voxel, TRUNC, dev(valid), dev(w), **kw)
    assert same_bits(plain[0], got[0]) and same_bits(plain[1], got[1])
    # a second run from the same start is bit-identical
    again = color.volume_integrate(*start(), d.to(DEV), c.to(DEV), Q, T, origin, voxel, TRUNC, dev(valid), dev(w), **kw)
    assert all(same_bits(a, g) for a, g in zip(again, got))
    return want


@pytest.mark.parametrize("case", CASES, ids=["%s-%s-V%d%s%s-A%d" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2], "p" if c[3] else "s",
                                                                    "+planes" if c[4] else "", c[5]) for c in CASES])
def test_integrate_against_the_restatement(ecm, case):
    want = run_integrate(ecm, case)
    dims, (H, W) = case[0], case[1]
    if min(dims) > 2 and min(H, W) > 2:
        touched, coloured = want[4], want[5]
        assert 0 < int(coloured.sum()) <= int(touched.sum()) < touched.numel()
        if case[5] >= 3:                                                   # with three planes or more some voxel reads a NaN or an Inf
            assert int(coloured.sum()) < int(touched.sum())                # ... so every outcome occurs
    ecm.ops.check_async_errors()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_integrate_with_attr_off_alignment_takes_the_scalar_path(ecm, offset):
    want = run_integrate(ecm, ((9, 6, 68), (40, 64), 3, True, True, 3), offset)
    assert int(want[5].sum()) > 0
    ecm.ops.check_async_errors()


def test_views_in_one_call_are_calls_in_order(ecm):
    ops, color = ecm.ops, ecm.color
    dims, (H, W) = (9, 6, 68), (40, 64)
    origin, voxel = box(dims)
    d, Q, (valid, w) = views(3, H, W, 5, True)
    c = dirty_attributes(3, 4, H, W, 6)
    T = torch.stack(POSES)
    new = lambda: ops.volume_new(dims, DEV) + color.volume_attributes_new(dims, 4, DEV)          # noqa: E731
    one = color.volume_integrate(*new(), d.to(DEV), c.to(DEV), Q, T, origin, voxel, TRUNC, valid.to(DEV), w.to(DEV))
    vol = new()
    assert vol[2].shape == (4,) + dims and vol[3].shape == dims and not bool(vol[2].any()) and not bool(vol[3].any())
    for v in range(3):
        color.volume_integrate(*vol, d[v:v + 1].to(DEV), c[v:v + 1].to(DEV), Q, T[v], origin, voxel, TRUNC, valid[v:v + 1].to(torch.uint8).to(DEV),
                               w[v:v + 1].to(DEV))
    assert all(same_bits(a, b) for a, b in zip(one, vol))
    assert bool((one[3] > 0).any()) and bool((one[3] == 0).any())
    # [V,1,H,W] planes are the same views
    four = color.volume_integrate(*new(), d[:, None].to(DEV), c.to(DEV), Q, T, origin, voxel, TRUNC, valid[:, None].to(DEV), w[:, None].to(DEV))
    assert all(same_bits(a, b) for a, b in zip(four, one))


# ---- raycast ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_volume():
    """The coloured loop volume with A = 1, 3 and 4 planes, a fifth of its coloured voxels uncoloured again so that the hits meet
    corners with asum == 0: {A: ((tsdf, wsum, attr, asum) on the device, the same on the CPU)}."""
    loop = color_loop()
    g = torch.Generator().manual_seed(9)
    asum = torch.where(torch.rand(DIMS, generator=g) < 0.2, torch.zeros(()), loop["asum"])
    extra = torch.rand((1,) + DIMS, generator=g)
    out = {}
    for A in (1, 3, 4):
        attr = (torch.cat([loop["attr"], extra]) if A == 4 else loop["attr"][:A]).contiguous()
        cpu = (loop["tsdf"], loop["wsum"], attr, asum)
        out[A] = (tuple(t.to(DEV) for t in cpu), cpu)
    return out


def compare_cast(ecm, vol_dev, vol, Q_out, T, size, near, far, step, label, **kw):
    ops, color = ecm.ops, ecm.color
    m = ops.volume_matrices(Q_out, T, ORIGIN, VOXEL)
    want = raycast_color_t(*vol, m.R, m.Rinv, size, near, far, step, **kw)
    out, colors, hw = color.volume_raycast(*vol_dev, Q_out, T, ORIGIN, VOXEL, size, near, far, step, with_weight=True, **kw)
    B, A = (T.shape[0] if T.dim() == 3 else 1), vol[2].shape[0]
    assert out.shape == hw.shape == (B, 1) + tuple(size) and colors.shape == (B, A) + tuple(size) and colors.dtype == F32
    hit = want["hit"]
    out_c, hw_c, col_c = out.cpu()[:, 0], hw.cpu()[:, 0], colors.cpu()
    assert torch.equal(out_c > 0, hit), label                              # holes are equal as sets
    assert bool((bits(col_c).permute(1, 0, 2, 3)[:, ~hit] == 0).all()), label                    # a hole is +0.0 in every plane
    seen = (ulps(out_c, want["out"]), ulps(hw_c, want["hit_weight"]), ulps(col_c, want["colors"]))
    print("raycast", label, "A", A, "hits", int(hit.sum()), "of", hit.numel(), "ulps (out, hit_weight, colors)", seen)
    assert max(seen) <= 1, (label, seen)
    # out and hit_weight are ops.volume_raycast's on the device, bit for bit
    plain = ops.volume_raycast(vol_dev[0], vol_dev[1], Q_out, T, ORIGIN, VOXEL, size, near, far, step, with_weight=True, **kw)
    assert same_bits(plain[0], out) and same_bits(plain[1], hw), label
    # without the weight; and a second run
    alone = color.volume_raycast(*vol_dev, Q_out, T, ORIGIN, VOXEL, size, near, far, step, **kw)
    assert len(alone) == 2 and same_bits(alone[0], out) and same_bits(alone[1], colors), label
    return want, col_c


@pytest.mark.parametrize("size", [(2, 2), (37, 61), (40, 64)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("step,A", [(0.25, 3), (0.5, 1), (0.5, 4), (1.0, 3)])
def test_raycast_against_the_restatement(ecm, loop_volume, size, step, A):
    vol_dev, vol = loop_volume[A]
    H, W = size
    Q_out = scene_q(H, W)
    fb = 1.25 * W * 0.25                                                   # scene_q's focal length times its baseline: d = fb / z
    want, col = compare_cast(ecm, vol_dev, vol, Q_out, FIFTH, size, fb / 1.6, fb / 5.0, step, f"{size} step {step}, one view")
    if min(size) > 2:
        assert float(want["hit"].to(F64).mean()) >= HIT_SHARE
    three, col3 = compare_cast(ecm, vol_dev, vol, Q_out, torch.stack([FIFTH] + POSES[:2]), size, fb / 1.6, fb / 5.0, step,
                               f"{size} step {step}, three views")
    assert torch.equal(bits(col3[0]), bits(col[0]))
    # view b of the batch is the single-view call, in all three outputs
    color = ecm.color
    batch = color.volume_raycast(*vol_dev, Q_out, torch.stack([FIFTH] + POSES[:2]), ORIGIN, VOXEL, size, fb / 1.6, fb / 5.0, step, with_weight=True)
    for b, T in enumerate([FIFTH] + POSES[:2]):
        alone = color.volume_raycast(*vol_dev, Q_out, T, ORIGIN, VOXEL, size, fb / 1.6, fb / 5.0, step, with_weight=True)
        assert all(same_bits(a[0], t[b]) for a, t in zip(alone, batch)), b


def test_raycast_from_inside_the_box_and_a_view_that_misses(ecm, loop_volume):
    vol_dev, vol = loop_volume[3]
    Q = scene_q(H0, W0)
    inside, _ = compare_cast(ecm, vol_dev, vol, Q, FIFTH, (H0, W0), 20.0 / 2.2, 20.0 / 3.4, 0.5, "starting and ending inside the box")
    assert 0.3 < float(inside["hit"].to(F64).mean()) < 1.0
    away = rigid(0.0, 3.0, 0.0, 0.0, 0.0, 0.0)                             # turned by 3 rad about y: the volume is behind the camera
    miss, col = compare_cast(ecm, vol_dev, vol, Q, away, (H0, W0), NEAR, FAR, 0.5, "a view that misses the box")
    assert not bool(miss["hit"].any()) and bool((bits(col) == 0).all())
    other, _ = compare_cast(ecm, vol_dev, vol, ecm.ops.q_matrix(70.0, 0.3, 30.0, 21.0), POSES[0], (37, 61), 14.0, 4.0, 0.7, "another Q_out",
                            max_steps=300)
    assert bool(other["hit"].any())


# ---- sample -----------------------------------------------------------------------------------------------------------------------------
def sample_points(N, dims, seed):
    """N world points about the grid of `dims` placed by box(dims): nodes, faces of the box, both sides of the half-voxel margin,
    NaN and Inf, and random points in and around the box."""
    origin, voxel = box(dims)
    nz, ny, nx = dims
    g = torch.Generator().manual_seed(seed)
    top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=F64)
    grid = (torch.rand(N, 3, generator=g, dtype=F64) * 1.3 - 0.15) * top   # 15 % beyond the box on every side
    k = min(N, 40)
    special = torch.stack([torch.randint(0, n, (k,), generator=g) for n in (nx, ny, nz)], 1).to(F64)      # nodes
    special[k // 4:k // 2, 0] = torch.where(torch.arange(k // 2 - k // 4) % 2 == 0, 0.0, float(nx - 1))   # ... on two faces
    margin = torch.tensor([-0.5, -0.5 - 1e-3, -0.5 + 1e-3, nx - 0.5, nx - 0.5 + 1e-3, nx - 0.5 - 1e-3], dtype=F64)
    special[k // 2:3 * k // 4, 0] = margin[torch.arange(3 * k // 4 - k // 2) % 6]
    special[3 * k // 4:k, 1] = torch.tensor([ny - 0.5 - 1e-3, ny - 0.5 + 1e-3, -0.5 + 1e-3, -0.5 - 1e-3], dtype=F64)[torch.arange(k - 3 * k // 4) % 4]
    grid[:k] = special
    pts = (torch.tensor(origin, dtype=F64) + voxel * grid).to(F32)
    for i, bad in enumerate((NAN, INF, -INF)):
        if N > 50 + i:
            pts[45 + i, i] = bad
    return pts, origin, voxel


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 5000])
@pytest.mark.parametrize("A", [1, 3, 4])
def test_sample_against_the_restatement(ecm, N, A):
    color, mesh = ecm.color, ecm.mesh
    dims = (6, 7, 12)
    attr, asum = used_attributes(dims, A, 21 + A)
    pts, origin, voxel = sample_points(N, dims, 100 + N)
    for T in (None, POSES[0]):
        want = sample_t(attr, asum, torch.linalg.inv(mesh.mesh_matrix(origin, voxel, T)), pts)
        got = color.volume_sample(attr.to(DEV), asum.to(DEV), pts.to(DEV), origin, voxel, T)
        assert got.shape == (N, A) and got.dtype == F32 and got.is_cuda
        seen = ulps(got.cpu(), want)
        print("sample N", N, "A", A, "T" if T is not None else "world", "zero rows", int((want == 0).all(1).sum()), "ulps", seen)
        assert seen <= 1 and torch.equal(got.cpu() == 0, want == 0)
        assert same_bits(color.volume_sample(attr.to(DEV), asum.to(DEV), pts.to(DEV), origin, voxel, T), got)
    if N == 5000:
        zero = (want == 0).all(1)
        assert 0.1 * N < int(zero.sum()) < 0.9 * N                         # inside and outside both occur
    ecm.ops.check_async_errors()


def test_mesh_colors_of_the_loop_volume(ecm):
    color, mesh = ecm.color, ecm.mesh
    loop = color_loop()
    vol = tuple(loop[k].to(DEV) for k in ("tsdf", "wsum", "attr", "asum"))
    for T in (None, FIFTH):
        m = mesh.volume_mesh(vol[0], vol[1], ORIGIN, VOXEL, T)
        got = color.mesh_colors(m, vol[2], vol[3], ORIGIN, VOXEL, T).cpu()
        want = sample_t(loop["attr"], loop["asum"], torch.linalg.inv(mesh.mesh_matrix(ORIGIN, VOXEL, T)), m.vertices.cpu())
        seen = ulps(got, want)
        world = m.vertices.cpu().to(F64).t()
        if T is not None:
            world = (torch.linalg.inv(T) @ torch.cat([world, torch.ones(1, world.shape[1], dtype=F64)]))[:3]
        err = float((got.to(F64) - affine_colors(world).t()).abs().mean())
        print("mesh colours: N", len(got), "frame", "world" if T is None else "FIFTH", "ulps", seen, "mean |c - truth|", err)
        assert got.shape == (m.vertices.shape[0], 3) and len(got) > 1000 and seen <= 1 and bool((got > 0).all())
        assert err <= VERTEX_COLOR_BOUND, err
    assert color.mesh_colors(mesh.Mesh(m.vertices[:0], m.faces[:0], None, None), vol[2], vol[3], ORIGIN, VOXEL).shape == (0, 3)   # an empty mesh


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_around_every_output(ecm):
    ops, color = ecm.ops, ecm.color
    for dims, (H, W), V, A in (((3, 5, 7), (37, 61), 3, 3), ((4, 4, 64), (40, 64), 1, 4), ((5, 5, 65), (40, 64), 3, 1), ((9, 6, 68), (2, 2), 3, 4),
                               ((1, 1, 1), (2, 2), 1, 3)):
        origin, voxel = box(dims)
        d, Q, (valid, w) = views(V, H, W, 11, True)
        c = dirty_attributes(V, A, H, W, 12)
        with guarded(ecm) as g:
            vol = ops.volume_new(dims, DEV) + color.volume_attributes_new(dims, A, DEV)
            assert len(g.records) == 4                                     # tsdf, wsum, attr, asum
            color.volume_integrate(*vol, d.to(DEV), c.to(DEV), Q, torch.stack(POSES[:V]), origin, voxel, TRUNC, valid.to(DEV), w.to(DEV))
            g.check(f"color.volume_integrate {dims}")
            assert len(g.records) == 4                                     # no scratch
            if min(dims) >= 2:
                for size in ((2, 2), (37, 61), (17, 16)):
                    color.volume_raycast(*vol, Q, torch.stack(POSES), origin, voxel, size, 12.0, 4.0, with_weight=True)
                g.check(f"color.volume_raycast {dims}")
                assert len(g.records) == 4 + 9                             # out, colors, hit_weight, three times
                for N in (1, 65, 1000):
                    pts, _, _ = sample_points(N, dims, N)
                    color.volume_sample(vol[2], vol[3], pts.to(DEV), origin, voxel)
                g.check(f"color.volume_sample {dims}")
                assert len(g.records) == 4 + 9 + 3
    ops.check_async_errors()


# ---- the closed loop and the mapper -----------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_device(ecm):
    ops, color = ecm.ops, ecm.color
    loop = color_loop()
    disp, Q = scene_views()
    vol = ops.volume_new(DIMS, DEV) + color.volume_attributes_new(DIMS, 3, DEV)
    color.volume_integrate(*vol, disp.to(DEV), scene_colors().to(DEV), Q, torch.stack(VIEWS), ORIGIN, VOXEL, TRUNC)
    seen = tuple(ulps(v.cpu(), loop[k]) for v, k in zip(vol, ("tsdf", "wsum", "attr", "asum")))
    out, colors = color.volume_raycast(*vol, Q, FIFTH, ORIGIN, VOXEL, (H0, W0), NEAR, FAR)
    out, colors = out.cpu()[0, 0], colors.cpu()[0]
    hit = out > 0
    err = color_error(colors, loop["truth"], hit)
    print("colour loop on the device: hit share", float(hit.to(F64).mean()), "mean |c - truth|", err, "volume ulps", seen,
          "raycast ulps", ulps(colors, loop["cast"]["colors"][0]))
    assert max(seen) <= 1 and torch.equal(hit, loop["cast"]["hit"][0]) and float(hit.to(F64).mean()) >= HIT_SHARE
    assert bool((colors[:, hit] > 0).all()) and bool((bits(colors[:, ~hit]) == 0).all())        # the colour holes are the disparity holes
    assert err <= COLOR_BOUND, err


def test_color_stereo_mapper_against_a_plain_mapper(ecm):
    """models.ColorStereoMapper driven by known maps (the Stub of tests/test_hip_motion_align.py in the network's place, its own
    odometry) beside a plain StereoMapper fed the same frames: the same Mapped, tsdf and wsum, bit for bit; the colours of the
    held-out view within the CPU loop's recorded bounds; the coloured mesh; reset()."""
    from test_hip_motion_align import Stub
    ops, models, color = ecm.ops, ecm.models, ecm.color
    maps, Q = mapper_maps()
    poses = mapper_poses()
    dev_maps = [m[None, None].to(DEV) for m in maps]
    images = scene_colors(poses).to(DEV)                                   # the colour image of every frame, as `colors`
    kw = dict(min_disp=MAPPER_MIN_DISP, step=1)
    mapper = models.ColorStereoMapper(ecm.get_model("cmfsm"), Q, ORIGIN, VOXEL, DIMS, TRUNC, **kw)
    plain = models.StereoMapper(ecm.get_model("cmfsm"), Q, ORIGIN, VOXEL, DIMS, TRUNC, **kw)
    mapper.odometry.tracker.model = Stub(dev_maps, MAPPER_STD)
    plain.odometry.tracker.model = Stub(dev_maps, MAPPER_STD)
    x = torch.zeros(1, 3, H0, W0, device=DEV)
    for k in range(len(poses)):
        a, b = mapper(x, x, colors=images[k:k + 1]), plain(x, x)
        assert isinstance(a, models.Mapped) and a.integrated and a.frames == k + 1
        for name in models.Mapped._fields:
            u, v = getattr(a, name), getattr(b, name)
            if isinstance(u, torch.Tensor):
                assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v), (k, name)
            elif name != "estimate":
                assert u == v, (k, name)
        assert (a.estimate is None) == (b.estimate is None) and (a.estimate is None or torch.equal(a.estimate.T, b.estimate.T))
    assert same_bits(mapper.volume[0], plain.volume[0]) and same_bits(mapper.volume[1], plain.volume[1])
    assert mapper.attributes[0].shape == (3,) + DIMS and bool((mapper.attributes[1] > 0).any())
    held = MAPPER_HELD_OUT                                                 # off the path: no view was taken here
    out, colors, hw = mapper.render_colors(T=held, near_disp=NEAR, far_disp=FAR, with_weight=True)
    both = plain.render(T=held, near_disp=NEAR, far_disp=FAR, with_weight=True)
    assert same_bits(out, both[0]) and same_bits(hw, both[1]) and colors.shape == (1, 3, H0, W0)
    hit = out.cpu()[0, 0] > 0
    # the truth is the affine colour of the true scene seen from `held`; the volume was filled at the poses the mapper estimated, so
    # the error carries their drift, as the reference loop's does (tests/test_volume_color_cpu.py::color_mapper_loop: its bounds)
    err = color_error(colors.cpu()[0], affine_colors(world_points(held, H0, W0, Q)), hit)
    print("colour mapper: hit share", float(hit.to(F64).mean()), "mean |c - truth|", err)
    assert float(hit.to(F64).mean()) >= HIT_SHARE and err <= MAPPER_COLOR_BOUND, err
    here = mapper.render_colors()
    assert len(here) == 2 and here[0].shape == (1, 1, H0, W0) and here[1].shape == (1, 3, H0, W0) and same_bits(here[0], plain.render())
    m, vc = mapper.colored_mesh()
    pm = plain.mesh()
    assert same_bits(m.vertices, pm.vertices) and torch.equal(m.faces, pm.faces) and vc.shape == (m.vertices.shape[0], 3)
    verr = float((vc.cpu().to(F64) - affine_colors(m.vertices.cpu().to(F64).t()).t()).abs().mean())
    print("colour mapper: vertices", len(vc), "mean |c - truth|", verr)
    assert len(vc) > 1000 and verr <= MAPPER_VERTEX_COLOR_BOUND, verr
    m2, vc2 = mapper.colored_mesh(T=held)
    # the same grid positions up to the fp32 rounding of the vertices in either frame: 3 m * 2^-24 is 3e-6 voxels, and a colour
    # moves by less than 0.02 per voxel
    assert vc2.shape == vc.shape and float((vc2 - vc).abs().max()) <= 1e-6
    mapper.reset()
    assert mapper.frames == 0 and bool((mapper.volume[0] == 1).all()) and all(not bool(t.any()) for t in (mapper.volume[1],) + tuple(mapper.attributes))
    ops.check_async_errors()


def test_color_stereo_mapper_smoke(ecm):
    ops, models = ecm.ops, ecm.models
    hw = (256, 512)
    torch.manual_seed(5)
    model = ecm.get_model("cmfsm").to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    frames = [(torch.randn(1, 3, *hw, device=DEV, generator=gen), torch.randn(1, 3, *hw, device=DEV, generator=gen)) for _ in range(2)]
    Q = ops.q_matrix(700.0, 0.25, 0.5 * hw[1], 0.5 * hw[0])
    motion = rigid(0.002, -0.003, 0.001, 0.01, 0.0, -0.05)
    args = (model, Q, (-2.0, -1.0, 0.5), 0.0625, (64, 32, 64), 0.25)
    mapper, plain = models.ColorStereoMapper(*args, min_disp=0.5), models.StereoMapper(*args, min_disp=0.5)
    for k, (left, right) in enumerate(frames):
        a, b = mapper(left, right, motion=motion), plain(left, right, motion=motion)    # colors None: the left image, as given
        for name in models.Tracked._fields:
            assert same_bits(getattr(a, name), getattr(b, name)), (k, name)
        assert a.integrated and a.frames == k + 1 and torch.equal(a.world, b.world)
    assert same_bits(mapper.volume[0], plain.volume[0]) and same_bits(mapper.volume[1], plain.volume[1])
    attr, asum = mapper.attributes
    assert attr.shape == (3, 64, 32, 64) and bool(torch.isfinite(attr).all()) and bool((asum >= 0).all()) and bool((asum <= mapper.volume[1]).all())
    out, colors = mapper.render_colors()
    assert out.shape == (1, 1) + hw and colors.shape == (1, 3) + hw and bool(torch.isfinite(colors).all()) and same_bits(out, plain.render())
    assert bool((colors[:, :, out[0, 0] == 0] == 0).all())
    mapper.reset()
    assert not bool(attr.any()) and not bool(asum.any()) and bool((mapper.volume[0] == 1).all())
    ops.check_async_errors()
