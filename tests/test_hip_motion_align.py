"""ops.motion_normal, ops.motion_estimate and models.StereoOdometry on the MI355X against align_t of
tests/test_motion_align_cpu.py, run on the CPU.

Each of the 29 sums is within the header's n * 2^-52 * sum |term| of the restatement (the bound of a reordered fp64 sum: the
per-pixel terms themselves are the same IEEE operations in the same order, without fused multiply-adds); the two counts are
equal; the residual plane is compared bit for bit where it is a number and as NaN elsewhere (observed: bit-equal on every case
here, so no ulp of slack is given).  Shapes: 2x2, 40x64, 37x61 (a partial last tile), steps 1, 2, 3, tile counts 1, 7, 8, 9 and
33 (every remainder of the finishing loop), and a batch of three with a shared and a per-image T."""
import ctypes as C

import pytest
import torch

from test_disp_warp_cpu import bits, rigid
from test_hip_guard_bands import POISON, guarded
from test_motion_align_cpu import F64, PLANES, POSE_BOUND, TRUE_MOTION, align_t, pose_error, render, restated, scene_pair, scene_q, tiles

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
NEAR = rigid(0.004, 0.011, -0.002, 0.04, -0.015, 0.05)


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def pair(B, H, W, seed, dirty=True):
    """Two maps of the three-plane scene, image b seen under its own small motion, with 0.01 px of noise; where dirty, NaN, inf,
    zero and negative disparities, invalid pixels and weights that are NaN, inf, zero or negative are strewn over both."""
    g = torch.Generator().manual_seed(seed)
    Q = scene_q(H, W)
    eye = torch.eye(4, dtype=F64)
    d0 = torch.stack([render(eye, H, W, PLANES, Q) for _ in range(B)]).to(torch.float32)
    d1 = torch.stack([render(rigid(0.001 * b, 0.003, 0.0, 0.01 * (b + 1), 0.0, 0.02), H, W, PLANES, Q) for b in range(B)]).to(torch.float32)
    d0, d1 = d0 + 0.01 * torch.randn(B, H, W, generator=g), d1 + 0.01 * torch.randn(B, H, W, generator=g)
    w = 0.5 + torch.rand(B, H, W, generator=g)
    v0, v1 = torch.rand(B, H, W, generator=g) > 0.05, torch.rand(B, H, W, generator=g) > 0.02
    if dirty:
        for t, values in ((d0, (NAN, INF, -INF, 0.0, -2.0)), (d1, (NAN, INF, 0.0)), (w, (NAN, INF, -INF, 0.0, -1.0))):
            r = torch.rand(B, H, W, generator=g)
            for k, bad in enumerate(values):
                t[(r >= 0.004 * k) & (r < 0.004 * (k + 1))] = bad
    return d0, d1, w, v0, v1, Q


def check(ops, d0, d1, Q, T, label, **kw):
    """One motion_normal call against align_t; returns (device sums, restatement)."""
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k in ("valid0", "valid1", "weight") else v) for k, v in kw.items()}
    sums, residual = ops.motion_normal(d0.to(DEV), d1.to(DEV), Q, T, with_residual=True, **dev)
    want = align_t(d0, d1, Q, T, **kw)
    got = sums.cpu()
    assert got.shape == want["sums"].shape and got.dtype == F64 and residual.shape == (d0.shape[0], 1) + tuple(d0.shape[1:])
    assert torch.equal(got[:, 29:], want["sums"][:, 29:]), (label, got[:, 29:], want["sums"][:, 29:])
    err = (got - want["sums"]).abs()
    over = err > want["bound"]
    assert not bool(over.any()), (label, over.nonzero().tolist(), float((err / want["bound"].clamp(min=1e-300))[over].max()))
    res = residual.cpu()[:, 0]
    nan = torch.isnan(want["residual"])
    assert torch.equal(torch.isnan(res), nan), label
    assert torch.equal(bits(res[~nan]), bits(want["residual"][~nan])), label
    return got, want


SHAPES = [(1, 2, 2), (1, 40, 64), (1, 37, 61), (2, 112, 128), (1, 128, 128), (1, 129, 128), (1, 263, 256)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("step", [1, 2, 3])
def test_sums_against_the_restatement(ecm, shape, step):
    B, H, W = shape
    d0, d1, w, v0, v1, Q = pair(B, H, W, 7 * H + W, dirty=min(H, W) > 2)
    got, want = check(ecm.ops, d0, d1, Q, NEAR if min(H, W) > 2 else torch.eye(4, dtype=F64), f"{shape} step {step}", valid0=v0, valid1=v1,
                      weight=w, step=step)
    if min(H, W) > 8:
        assert bool((want["sums"][:, 29] > 0.5 * want["sums"][:, 30]).all()) and bool((want["sums"][:, 30] > 0.6 * (H // step) * (W // step)).all())
    if step == 1:
        assert tiles(H, W, 1) == {(2, 2): 1, (40, 64): 2, (37, 61): 2, (112, 128): 7, (128, 128): 8, (129, 128): 9, (263, 256): 33}[(H, W)]
    # without the optional planes
    check(ecm.ops, d0, d1, Q, NEAR, f"{shape} step {step}, no planes", step=step)


def test_batch_of_three_shared_and_per_image(ecm):
    ops = ecm.ops
    d0, d1, w, v0, v1, Q = pair(3, 40, 64, 3)
    Ts = torch.stack([NEAR, torch.eye(4, dtype=F64), rigid(-0.002, 0.001, 0.003, -0.01, 0.02, 0.0)])
    kw = dict(valid0=v0, valid1=v1, weight=w)
    shared, _ = check(ops, d0, d1, Q, NEAR, "shared T", **kw)
    per, _ = check(ops, d0, d1, Q, Ts, "per-image T", **kw)
    assert torch.equal(per[0], shared[0]) and not torch.equal(per[1], shared[1])
    # two runs are bit-equal, and image b alone is image b of the batch
    again = ops.motion_normal(d0.to(DEV), d1.to(DEV), Q, Ts, v0.to(DEV), v1.to(DEV), w.to(DEV), with_residual=True)
    first = ops.motion_normal(d0.to(DEV), d1.to(DEV), Q, Ts, v0.to(DEV), v1.to(DEV), w.to(DEV), with_residual=True)
    assert torch.equal(again[0].view(torch.int64), first[0].view(torch.int64)) and torch.equal(bits(again[1]), bits(first[1]))
    assert torch.equal(again[0].cpu(), per)
    for b in range(3):
        alone = ops.motion_normal(d0[b:b + 1].to(DEV), d1[b:b + 1].to(DEV), Q, Ts[b], v0[b:b + 1].to(DEV), v1[b:b + 1].to(DEV),
                                  w[b:b + 1].to(DEV), with_residual=True)
        assert torch.equal(alone[0].view(torch.int64), first[0][b:b + 1].view(torch.int64)), b
        assert torch.equal(bits(alone[1]), bits(first[1][b:b + 1])), b
    # a Q_out of its own, and a uint8 mask
    Q_out = ops.q_matrix(1.2 * 64, 0.25, 31.0, 20.5)
    check(ops, d0, d1, Q, Ts, "Q_out", Q_out=Q_out, valid0=v0.to(torch.uint8), max_disp=7.5, min_disp=6.6, cauchy=0.02, max_residual=0.5)


def test_the_last_row_and_column_and_a_depth_edge(ecm):
    ops = ecm.ops
    eye = torch.eye(4, dtype=F64)
    Qp = ops.q_matrix(64.0, 0.25, 4.0, 2.0)                                # powers of two: the identity lands on the pixel itself
    d = torch.full((1, 4, 6), 4.0)
    d[0, :, 3:] = 8.0                                                      # a depth edge between columns 2 and 3
    got, want = check(ops, d, d, Qp, eye, "edge")
    assert torch.equal(want["u"][0, 0], torch.arange(6, dtype=F64)) and float(want["u"][0, 0, -1]) == 5.0   # u == W-1: x0 = W-2, fx = 1
    assert got[0, 29:31].tolist() == [20.0, 24.0]                          # column 2 straddles the edge: fx = 0, but the taps differ
    got, _ = check(ops, d, d, Qp, eye, "edge, wide", tap_range=4.0)
    assert got[0, 29:31].tolist() == [24.0, 24.0] and float(got[0, 27]) == 0.0
    smooth = torch.full((1, 4, 6), 4.0) + 0.125 * torch.arange(6) + 0.25 * torch.arange(4)[:, None]
    got, want = check(ops, smooth, smooth, Qp, eye, "ramp")
    assert float(got[0, 30]) >= 8 and float(want["gx"][0, 1, 2]) == pytest.approx(0.125, abs=1e-12) \
        and float(want["gy"][0, 1, 2]) == pytest.approx(0.25, abs=1e-12)


def test_guard_bands_and_the_short_scratch(ecm):
    ops, lib = ecm.ops, ecm._lib
    for B, H, W in SHAPES[:4]:
        d0, d1, w, v0, v1, Q = pair(B, H, W, 11)
        for step, with_residual in ((1, True), (2, True), (3, False)):
            with guarded(ecm) as g:
                ops.motion_normal(d0.to(DEV), d1.to(DEV), Q, NEAR, v0.to(DEV), v1.to(DEV), w.to(DEV), step=step, with_residual=with_residual)
                g.check(f"motion_normal {(B, H, W)} step {step}")
                assert len(g.records) == 2 + with_residual                 # sums, [residual,] the partials
    B, H, W = 3, 37, 61
    d0, d1, _, _, _, Q = pair(B, H, W, 13)
    d0, d1 = d0.to(DEV), d1.to(DEV)
    nb = int(lib.query("ecmm_align_scratch_bytes", B, H, W, 1))
    assert nb == B * 2 * 256
    mats = torch.cat([Q.reshape(-1), torch.linalg.inv(Q).reshape(-1), NEAR.reshape(-1)]).to(DEV)
    sums, partial = (torch.full((s,), POISON, dtype=torch.uint8, device=DEV) for s in (B * 256, nb))
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                                          # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda n: (p(d0), None, None, p(d1), None, p(mats), p(mats, 128), p(mats, 256), 0, p(sums), None, p(partial),  # noqa: E731
                      C.c_longlong(n), B, H, W, 1, 0.0, INF, 1.0, 3.0, 1.0, st)
    with pytest.raises(RuntimeError, match="scratch"):
        lib.call("ecmm_align_normal_fwd", *args(nb - 1))
    torch.cuda.synchronize()
    assert all(bool((t == POISON).all()) for t in (sums, partial))
    lib.call("ecmm_align_normal_fwd", *args(nb))
    torch.cuda.synchronize()
    want = align_t(d0.cpu(), d1.cpu(), Q, NEAR)
    assert torch.equal(sums.view(F64).view(B, 32)[:, 29:].cpu(), want["sums"][:, 29:])


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_motion_estimate_recovers_the_motion(ecm):
    ops = ecm.ops
    d0, d1, Q = scene_pair()
    est = ops.motion_estimate(d0.to(DEV), d1.to(DEV), Q)
    ref = ops.motion_estimate(d0, d1, Q, normal=restated(d0, d1, Q))
    err = pose_error(est.T[0], TRUE_MOTION)
    print("motion_estimate: pose error", err, "against the restatement's loop", float((est.T - ref.T).abs().max()))
    assert bool(est.converged[0]) and int(est.iterations[0]) == int(ref.iterations[0]) and int(est.used[0]) == int(ref.used[0])
    assert err <= POSE_BOUND, err
    assert not est.T.is_cuda and est.T.dtype == F64 and est.T.shape == (1, 4, 4)
    # nothing to align: init, not converged
    init = rigid(0.001, 0.002, 0.003, 0.01, 0.02, 0.03)
    none = ops.motion_estimate(torch.zeros(1, 40, 64, device=DEV), d1.to(DEV), Q, init=init)
    assert torch.equal(none.T[0], init) and not bool(none.converged[0]) and int(none.used[0]) == 0


class Stub(torch.nn.Module):
    """Stands where the network stands in a tracker: predict() hands out the next of a list of known disparity maps."""
    HEAD = "stub"

    def __init__(self, maps, std):
        super().__init__()
        self.maps, self.std, self.at = maps, std, 0

    def predict(self, left, right, heads):
        import collections
        d = self.maps[self.at]
        self.at += 1
        return collections.namedtuple("P", "disparity std")([d], [torch.full_like(d, self.std)])


def test_stereo_odometry_is_the_tracker_fed_the_estimate(ecm):
    models, ops = ecm.models, ecm.ops
    H, W = 40, 64
    Q = scene_q(H, W)
    step1 = rigid(0.003, 0.007, -0.002, 0.025, -0.01, 0.03)
    poses = [torch.eye(4, dtype=F64), step1, step1 @ step1]
    maps = [render(p, H, W, PLANES, Q).to(torch.float32)[None, None].to(DEV) for p in poses]
    net = ecm.get_model("cmfsm")
    odo, tracker = models.StereoOdometry(net, Q, step=1), models.DisparityTracker(net, Q)
    odo.tracker.model, tracker.model = Stub(maps, 0.05), Stub(maps, 0.05)
    x = torch.zeros(1, 3, H, W, device=DEV)
    for k in range(3):
        o = odo(x, x)
        t = tracker(x, x, motion=None if o.restarted else o.motion)
        assert o.restarted == (k == 0) and (o.estimate is None) == (k == 0)
        for name in models.Tracked._fields:
            a, b = getattr(o, name), getattr(t, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, name)
        if k:
            assert bool(o.estimate.converged.all()) and pose_error(o.motion[0], step1) <= POSE_BOUND, (k, pose_error(o.motion[0], step1))
            assert int((o.age == k + 1).sum()) > 0.8 * H * W               # the state was carried: most pixels fused again
        assert pose_error(o.pose[0], poses[k]) <= k * POSE_BOUND
    # an estimate that cannot converge starts over and says so
    odo.tracker.model = Stub([torch.zeros_like(maps[0])], 0.05)
    o = odo(x, x)
    assert o.restarted and o.estimate is not None and not bool(o.estimate.converged.any()) and torch.equal(o.pose[0], torch.eye(4, dtype=F64))
