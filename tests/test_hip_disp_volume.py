"""ops.volume_integrate, ops.volume_raycast and models.StereoMapper on the MI355X against integrate_t and
raycast_t of tests/test_disp_volume_cpu.py, run on the CPU.

The per-voxel and per-pixel arithmetic of the device is the restatement's, operation for operation (IEEE fp64 and fp32 without
fused multiply-adds), so bit-equality is expected; one ulp of fp32 is allowed, and every test prints the largest difference it
saw.  Holes of the raycast must be equal as sets.  Volumes: 1x1x1, 3x5x7, one brick of the 16-byte path exactly (4x4x64) and of
the 4-byte path plus one on each axis (5x5x17, 5x5x65), nx not a multiple of 4, a partial brick of the 16-byte path (4x4x16) and
one brick plus one thread (9x6x68); images 2x2, 37x61 and 40x64; one and three views with shared and per-view matrices."""
import pytest
import torch

from test_disp_warp_cpu import bits, rigid
from test_hip_guard_bands import guarded
from test_disp_volume_cpu import (DIMS, F32, F64, FAR, FIFTH, H0, HIT_SHARE, MAPPER_BOUND, MAPPER_HELD_OUT, MAPPER_MIN_DISP, MAPPER_STD, NEAR, ORIGIN,
                                  RAYCAST_BOUND, TRUNC, VIEWS, VOXEL, W0, closed_loop, integrate_t, loop_error, mapper_loop, mapper_maps, mapper_poses,
                                  raycast_t, scene_views)
from test_motion_align_cpu import PLANES, POSE_BOUND, pose_error, render, scene_q

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
POSES = [rigid(0.004, 0.011, -0.002, 0.04, -0.015, 0.05), torch.eye(4, dtype=F64), rigid(-0.01, 0.02, 0.0, -0.06, 0.03, -0.04)]


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def ulps(a, b):
    """The largest distance, in representable fp32 values, between two tensors without NaNs (+0.0 and -0.0 count as equal)."""
    key = lambda t: torch.where(bits(t) < 0, -(bits(t) & 0x7FFFFFFF), bits(t)).to(torch.int64)  # noqa: E731
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def box(dims):
    """(origin, voxel) of a grid of dims = (nz, ny, nx) centred 3 m in front of the first camera, 1.6 m along its longest side."""
    nz, ny, nx = dims
    voxel = 1.6 / max(max(dims) - 1, 1)
    return (-voxel * (nx - 1) / 2, -voxel * (ny - 1) / 2, 3.0 - voxel * (nz - 1) / 2), voxel


def views(V, H, W, seed, planes):
    """V dirty views of the three-plane scene and their optional planes (valid, weight)."""
    g = torch.Generator().manual_seed(seed)
    Q = scene_q(H, W)
    d = torch.stack([render(POSES[v], H, W, PLANES, Q) for v in range(V)]).to(F32) + 0.01 * torch.randn(V, H, W, generator=g)
    w = 0.5 + torch.rand(V, H, W, generator=g)
    valid = torch.rand(V, H, W, generator=g) > 0.05
    if min(H, W) > 2:
        for t, values in ((d, (NAN, INF, -INF, 0.0, -2.0)), (w, (NAN, INF, -INF, 0.0, -1.0))):
            r = torch.rand(V, H, W, generator=g)
            for k, bad in enumerate(values):
                t[(r >= 0.01 * k) & (r < 0.01 * (k + 1))] = bad
    return d, Q, (valid, w) if planes else (None, None)


def used_volume(dims, seed):
    """A volume that has seen views before: tsdf in [-1, 1], wsum in [0, 3] with a third of it empty."""
    g = torch.Generator().manual_seed(seed)
    tsdf = 2 * torch.rand(dims, generator=g) - 1
    wsum = 3 * torch.rand(dims, generator=g)
    fresh = torch.rand(dims, generator=g) < 0.33
    return torch.where(fresh, torch.ones(dims), tsdf), torch.where(fresh, torch.zeros(dims), wsum)


CASES = [((1, 1, 1), (2, 2), 1, False, False), ((3, 5, 7), (37, 61), 3, True, True), ((4, 4, 64), (40, 64), 1, False, True),
         ((5, 5, 65), (40, 64), 3, False, False), ((4, 4, 16), (37, 61), 3, True, False), ((5, 5, 17), (40, 64), 1, False, True),
         ((9, 6, 68), (40, 64), 3, True, True), ((6, 7, 10), (2, 2), 3, True, True), ((24, 20, 36), (37, 61), 3, False, True)]


@pytest.mark.parametrize("case", CASES, ids=["%s-%s-V%d%s%s" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2], "p" if c[3] else "s",
                                                                "+planes" if c[4] else "") for c in CASES])
def test_integrate_against_the_restatement(ecm, case):
    ops = ecm.ops
    dims, (H, W), V, per_view, planes = case
    origin, voxel = box(dims)
    d, Q, (valid, w) = views(V, H, W, 7 * H + W + V, planes)
    T = torch.stack(POSES[:V]) if per_view else POSES[0]
    kw = dict(max_weight=2.5, min_disp=0.05, max_disp=1.25 * W * 0.25 / 2.7)       # d = fb / z: nearer than 2.7 m is gated out
    tsdf0, wsum0 = used_volume(dims, sum(dims))
    m = ops.volume_matrices(Q, T, origin, voxel)
    X, N, touched = integrate_t(tsdf0, wsum0, d, Q, m.G, m.C, TRUNC, valid, w, **kw)
    tsdf, wsum = tsdf0.to(DEV), wsum0.to(DEV)
    dev = lambda t: None if t is None else t.to(DEV)                                            # noqa: E731
    back = ops.volume_integrate(tsdf, wsum, d.to(DEV), Q, T, origin, voxel, TRUNC, dev(valid), dev(w), **kw)
    assert back[0] is tsdf and back[1] is wsum                             # in place
    got_x, got_n = tsdf.cpu(), wsum.cpu()
    seen = (ulps(got_x, X), ulps(got_n, N))
    print("integrate", case, "touched", int(touched.sum()), "of", touched.numel(), "ulps (tsdf, wsum)", seen)
    assert max(seen) <= 1, seen
    assert torch.equal(bits(got_x)[~touched], bits(tsdf0)[~touched]) and torch.equal(bits(got_n)[~touched], bits(wsum0)[~touched])
    if min(dims) > 2 and min(H, W) > 2:
        assert 0.1 * touched.numel() < int(touched.sum()) < touched.numel()                     # the case exercises both outcomes
    # a second run from the same start is bit-identical
    again = ops.volume_integrate(tsdf0.to(DEV), wsum0.to(DEV), d.to(DEV), Q, T, origin, voxel, TRUNC, dev(valid), dev(w), **kw)
    assert torch.equal(bits(again[0].cpu()), bits(got_x)) and torch.equal(bits(again[1].cpu()), bits(got_n))
    ops.check_async_errors()


def test_views_in_one_call_are_calls_in_order_and_uint8_masks(ecm):
    ops = ecm.ops
    dims, (H, W) = (9, 6, 68), (40, 64)
    origin, voxel = box(dims)
    d, Q, (valid, w) = views(3, H, W, 5, True)
    T = torch.stack(POSES)
    one = ops.volume_integrate(*ops.volume_new(dims, DEV), d.to(DEV), Q, T, origin, voxel, TRUNC, valid.to(DEV), w.to(DEV))
    vol = ops.volume_new(dims, DEV)
    for v in range(3):
        ops.volume_integrate(*vol, d[v:v + 1].to(DEV), Q, T[v], origin, voxel, TRUNC, valid[v:v + 1].to(torch.uint8).to(DEV), w[v:v + 1].to(DEV))
    assert torch.equal(bits(one[0]), bits(vol[0])) and torch.equal(bits(one[1]), bits(vol[1]))
    assert bool((one[1] > 0).any()) and bool((one[1] == 0).any())
    # [V,1,H,W] planes are the same views
    four = ops.volume_integrate(*ops.volume_new(dims, DEV), d[:, None].to(DEV), Q, T, origin, voxel, TRUNC, valid[:, None].to(DEV), w[:, None].to(DEV))
    assert torch.equal(bits(four[0]), bits(one[0])) and torch.equal(bits(four[1]), bits(one[1]))


def test_guard_bands_around_both_planes_and_the_raycast(ecm):
    ops = ecm.ops
    for dims, (H, W), V in (((3, 5, 7), (37, 61), 3), ((4, 4, 64), (40, 64), 1), ((5, 5, 65), (40, 64), 3), ((9, 6, 68), (2, 2), 3), ((1, 1, 1), (2, 2), 1)):
        origin, voxel = box(dims)
        d, Q, (valid, w) = views(V, H, W, 11, True)
        with guarded(ecm) as g:
            vol = ops.volume_new(dims, DEV)
            ops.volume_integrate(*vol, d.to(DEV), Q, torch.stack(POSES[:V]), origin, voxel, TRUNC, valid.to(DEV), w.to(DEV))
            g.check(f"volume_integrate {dims}")
            assert len(g.records) == 2                                     # tsdf and wsum: no scratch
            if min(dims) >= 2:
                for size in ((2, 2), (37, 61), (17, 16)):
                    ops.volume_raycast(*vol, Q, torch.stack(POSES), origin, voxel, size, 12.0, 4.0, with_weight=True)
                g.check(f"volume_raycast {dims}")
                assert len(g.records) == 8
    ops.check_async_errors()


# ---- raycast ----------------------------------------------------------------------------------------------------------------------------
def compare_cast(ops, vol_dev, vol, Q_out, T, size, near, far, step, label, **kw):
    m = ops.volume_matrices(Q_out, T, ORIGIN, VOXEL)
    want = raycast_t(*vol, m.R, m.Rinv, size, near, far, step, **kw)
    out, hw = ops.volume_raycast(*vol_dev, Q_out, T, ORIGIN, VOXEL, size, near, far, step, with_weight=True, **kw)
    B = T.shape[0] if T.dim() == 3 else 1
    assert out.shape == hw.shape == (B, 1) + tuple(size) and out.dtype == F32
    out, hw = out.cpu()[:, 0], hw.cpu()[:, 0]
    assert torch.equal(out > 0, want["hit"]) and torch.equal(bits(out)[~want["hit"]], torch.zeros_like(bits(out))[~want["hit"]]), label
    assert torch.equal(hw > 0, want["hit"]) and bool((hw[~want["hit"]] == 0).all()), label
    seen = (ulps(out, want["out"]), ulps(hw, want["hit_weight"]))
    print("raycast", label, "hits", int(want["hit"].sum()), "of", want["hit"].numel(), "ulps (out, hit_weight)", seen)
    assert max(seen) <= 1, (label, seen)
    alone = ops.volume_raycast(*vol_dev, Q_out, T, ORIGIN, VOXEL, size, near, far, step, **kw)
    assert isinstance(alone, torch.Tensor) and torch.equal(bits(alone.cpu()[:, 0]), bits(out))   # without the weight; and a second run
    return want


@pytest.fixture(scope="module")
def loop_volume():
    loop = closed_loop()
    return (loop["tsdf"].to(DEV), loop["wsum"].to(DEV)), (loop["tsdf"], loop["wsum"])


@pytest.mark.parametrize("size", [(2, 2), (37, 61), (40, 64)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("step", [0.25, 0.5, 1.0])
def test_raycast_against_the_restatement(ecm, loop_volume, size, step):
    vol_dev, vol = loop_volume
    H, W = size
    Q_out = scene_q(H, W)
    fb = 1.25 * W * 0.25                                                   # scene_q's focal length times its baseline: d = fb / z
    want = compare_cast(ecm.ops, vol_dev, vol, Q_out, FIFTH, size, fb / 1.6, fb / 5.0, step, f"{size} step {step}, one view")
    if min(size) > 2:
        assert float(want["hit"].to(F64).mean()) >= HIT_SHARE
    three = compare_cast(ecm.ops, vol_dev, vol, Q_out, torch.stack([FIFTH] + POSES[:2]), size, fb / 1.6, fb / 5.0, step,
                         f"{size} step {step}, three views")
    assert torch.equal(bits(three["out"][0]), bits(want["out"][0]))


def test_raycast_from_inside_the_box_max_steps_and_a_view_that_misses(ecm, loop_volume):
    vol_dev, vol = loop_volume
    Q = scene_q(H0, W0)
    inside = compare_cast(ecm.ops, vol_dev, vol, Q, FIFTH, (H0, W0), 20.0 / 2.2, 20.0 / 3.4, 0.5, "starting and ending inside the box")
    assert 0.3 < float(inside["hit"].to(F64).mean()) < 1.0                 # z from 2.2 m to 3.4 m: some surfaces lie beyond the far end
    n = int(inside["n"].min())                                             # the shortest rays alone are marched
    few = compare_cast(ecm.ops, vol_dev, vol, Q, FIFTH, (H0, W0), 20.0 / 2.2, 20.0 / 3.4, 0.5, "max_steps below most rays", max_steps=n)
    assert int(few["hit"].sum()) < int(inside["hit"].sum()) and torch.equal(few["hit"], inside["hit"] & (inside["n"] <= n))
    away = rigid(0.0, 3.0, 0.0, 0.0, 0.0, 0.0)                             # turned by 3 rad about y: the volume is behind the camera
    miss = compare_cast(ecm.ops, vol_dev, vol, Q, away, (H0, W0), NEAR, FAR, 0.5, "a view that misses the box")
    assert not bool(miss["hit"].any())
    other = compare_cast(ecm.ops, vol_dev, vol, ecm.ops.q_matrix(70.0, 0.3, 30.0, 21.0), POSES[0], (37, 61), 14.0, 4.0, 0.7, "another Q_out")
    assert bool(other["hit"].any())


def test_closed_loop_on_the_device(ecm):
    ops = ecm.ops
    loop = closed_loop()
    disp, Q = scene_views()
    vol = ops.volume_new(DIMS, DEV)
    ops.volume_integrate(*vol, disp.to(DEV), Q, torch.stack(VIEWS), ORIGIN, VOXEL, TRUNC)
    seen = (ulps(vol[0].cpu(), loop["tsdf"]), ulps(vol[1].cpu(), loop["wsum"]))
    out = ops.volume_raycast(*vol, Q, FIFTH, ORIGIN, VOXEL, (H0, W0), NEAR, FAR).cpu()[0, 0]
    share, err = loop_error(out, loop["truth"])
    print("closed loop on the device: hit share", share, "mean |d - truth|", err, "volume ulps", seen,
          "raycast ulps", ulps(out, loop["cast"]["out"][0]))
    assert max(seen) <= 1 and share >= HIT_SHARE and err <= RAYCAST_BOUND, (seen, share, err)


def test_stereo_mapper_smoke(ecm):
    ops, models = ecm.ops, ecm.models
    hw = (256, 512)
    torch.manual_seed(5)
    model = ecm.get_model("cmfsm").to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    frames = [(torch.randn(1, 3, *hw, device=DEV, generator=gen), torch.randn(1, 3, *hw, device=DEV, generator=gen)) for _ in range(2)]
    Q = ops.q_matrix(700.0, 0.25, 0.5 * hw[1], 0.5 * hw[0])
    motion = rigid(0.002, -0.003, 0.001, 0.01, 0.0, -0.05)
    mapper = models.StereoMapper(model, Q, (-2.0, -1.0, 0.5), 0.0625, (64, 32, 64), 0.25, min_disp=0.5)
    tracker = models.DisparityTracker(model, Q)
    eye = torch.eye(4, dtype=F64)
    for k, (left, right) in enumerate(frames):
        m = mapper(left, right, motion=motion)
        t = tracker(left, right, motion=motion)
        assert isinstance(m, models.Mapped)
        for name in models.Tracked._fields:
            a, b = getattr(m, name), getattr(t, name)
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, name)
        assert torch.equal(m.motion[0], motion) and m.estimate is None and m.restarted == (k == 0) and m.integrated and m.frames == k + 1
        assert torch.equal(m.world, motion if k else eye) and torch.equal(m.pose[0], m.world)
    assert mapper.frames == 2 and bool((mapper.volume[1] >= 0).all()) and bool(torch.isfinite(mapper.volume[0]).all())
    out, hw_ = mapper.render(with_weight=True)
    assert out.shape == (1, 1) + hw and bool(torch.isfinite(out).all()) and bool((out >= 0).all()) and bool(torch.isfinite(hw_).all())
    other = mapper.render(T=eye, size=(64, 96), near_disp=200.0, far_disp=2.0, step=1.0)
    assert other.shape == (1, 1, 64, 96) and bool(torch.isfinite(other).all())
    mapper.reset()
    assert mapper.frames == 0 and bool((mapper.volume[0] == 1).all()) and bool((mapper.volume[1] == 0).all()) and torch.equal(mapper.world, eye)
    ops.check_async_errors()


def test_stereo_mapper_closes_the_loop(ecm):
    """models.StereoMapper driven by known maps (the Stub of tests/test_hip_motion_align.py in the network's place, motion=None:
    its own odometry), against the reference loop of tests/test_disp_volume_cpu.py: world = motion @ world, T world to camera,
    the frame's own disparity integrated.  Then a frame that cannot converge, and reset()."""
    from test_hip_motion_align import Stub
    ops, models = ecm.ops, ecm.models
    ref = mapper_loop()
    maps, Q = mapper_maps()
    poses = mapper_poses()
    dev_maps = [m[None, None].to(DEV) for m in maps]
    mapper = models.StereoMapper(ecm.get_model("cmfsm"), Q, ORIGIN, VOXEL, DIMS, TRUNC, min_disp=MAPPER_MIN_DISP, step=1)
    mapper.odometry.tracker.model = Stub(dev_maps, MAPPER_STD)
    x = torch.zeros(1, 3, H0, W0, device=DEV)
    eye = torch.eye(4, dtype=F64)
    errors = []
    for k in range(len(poses)):
        m = mapper(x, x)
        assert isinstance(m, models.Mapped) and m.integrated and m.frames == k + 1 and m.restarted == (k == 0), k
        assert (m.estimate is None) == (k == 0) and torch.equal(m.world, mapper.world) and m.world is not mapper.world
        assert torch.equal(m.disparity.view(torch.int32), dev_maps[k].view(torch.int32))
        errors.append(pose_error(m.world, poses[k]))
        assert errors[-1] <= k * POSE_BOUND, (k, errors)
    assert torch.equal(mapper.world, m.world) and mapper.frames == 5
    assert bool((mapper.volume[1] >= 0).all()) and bool(torch.isfinite(mapper.volume[0]).all())
    out, hw = mapper.render(T=MAPPER_HELD_OUT, near_disp=NEAR, far_disp=FAR, with_weight=True)
    assert out.shape == (1, 1, H0, W0) and bool(torch.isfinite(out).all()) and bool((out >= 0).all()) and bool(torch.isfinite(hw).all())
    share, err = loop_error(out.cpu()[0, 0], ref["truth"])
    ref_share, ref_err = loop_error(ref["cast"]["out"][0], ref["truth"])
    print("mapper on the device: pose errors", errors, "hit share", share, "mean |d - truth|", err, "(the reference loop:", ref_share, ref_err, ")")
    assert share >= HIT_SHARE and err <= MAPPER_BOUND, (share, err)
    here = mapper.render()                                                 # at the current pose, the last frame's size
    assert here.shape == (1, 1, H0, W0) and float((here > 0).to(F64).mean()) >= HIT_SHARE
    # a frame that cannot converge: not integrated, the pose and the count held, both planes bit-unchanged
    before = [t.clone() for t in mapper.volume]
    world = mapper.world.clone()
    mapper.odometry.tracker.model = Stub([torch.zeros_like(dev_maps[0])], MAPPER_STD)
    m = mapper(x, x)
    assert not m.integrated and m.restarted and m.frames == 5 and mapper.frames == 5 and torch.equal(m.world, world) and torch.equal(mapper.world, world)
    assert m.estimate is not None and not bool(m.estimate.converged.any())
    assert all(torch.equal(bits(t), bits(b)) for t, b in zip(mapper.volume, before))
    mapper.reset()
    assert mapper.frames == 0 and bool((mapper.volume[0] == 1).all()) and bool((mapper.volume[1] == 0).all()) and torch.equal(mapper.world, eye)
    ops.check_async_errors()
