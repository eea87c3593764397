"""The dense disparity alignment without a GPU: align_t, an fp64 torch restatement of include/ecm_motion.h
written from the header's text; the Jacobian against central differences; se3_exp / se3_log; ops.motion_estimate's own loop
driven by the restatement on a three-plane scene; the degenerate inputs; and the fifth header's census, refusal contract and
size query.  tests/test_hip_motion_align.py compares the device with align_t.

Every operation of align_t is one torch fp64 operation in the header's order (separate elementwise calls: nothing is fused), so
the per-pixel values are the header's bit for bit; only the order of the 31 sums is torch's own."""
import ctypes as C
import inspect
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import abi_refusal_child as child
from test_abi_refusals import EINVAL, EUNSUP, ESCRATCH, HIDE, Row, _report, calls_of, classify, classify_query, query_calls
from test_abi_types import INCLUDE, _strip, compare, lib_mod, package_entry_names, parse_header  # noqa: F401  (lib_mod: a fixture)
from test_disp_warp_cpu import rigid

HEADER = "ecm_motion.h"
PREFIX = "ecmm_"
ENTRIES = ("ecmm_align_normal_fwd", "ecmm_align_scratch_bytes", "ecmm_align_sums")
NAN, INF = float("nan"), float("inf")
FLT_MAX = 3.4028234663852886e38
F64 = torch.float64
TILE = 2048

# The pose error |se3_log(T_est T_true^-1)| (metres and radians in one norm) of the closed loop on the three-plane scene at 40x64
# with fp32-rounded maps: MEASURED is what the restatement reaches (printed by the test below; 10 Gauss-Newton steps from the
# identity), and the device, which differs from the restatement by the order of its sums only, is allowed POSE_BOUND = 10 x that.
MEASURED_POSE_ERROR = 4.3e-4
POSE_BOUND = 10 * MEASURED_POSE_ERROR


def ecm():
    import ecm_amd
    return ecm_amd


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _row(m, a, b, c):
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3]


def align_t(disp0, disp1, Q, T, valid0=None, valid1=None, weight=None, Q_out=None, step=1, min_disp=0.0, max_disp=None,
            tap_range=1.0, max_residual=3.0, cauchy=1.0):
    """include/ecm_motion.h on CPU tensors.  A dict: sums [B,32] fp64; residual [B,H,W] fp32; bound [B,32], the header's
    n * 2^-52 * sum |term| per entry; and the per-lattice-pixel planes used, cand, r, J [..,6], u, v (fp64, [B,Hs,Ws])."""
    B, H, W = disp0.shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)                                         # noqa: E731
    lo, hi = f32(min_disp), f32(FLT_MAX if max_disp is None else min(max_disp, FLT_MAX))
    A = torch.linalg.inv(Q if Q_out is None else Q_out)
    Tb = (T if T.dim() == 3 else T.expand(B, 4, 4)).reshape(B, 16, 1, 1)
    ok = lambda d, v: torch.isfinite(d) & v & (d > lo) & (d <= hi)                               # noqa: E731
    every = torch.ones(B, H, W, dtype=torch.bool)
    v0 = every if valid0 is None else valid0 != 0
    v1 = every if valid1 is None else valid1 != 0
    ys, xs = torch.meshgrid(torch.arange(0, H, step), torch.arange(0, W, step), indexing="ij")
    x, y = xs.to(F64).expand(B, -1, -1), ys.to(F64).expand(B, -1, -1)
    d = disp0[:, ::step, ::step]
    w = torch.ones_like(x) if weight is None else weight[:, ::step, ::step].to(F64)
    fd = d.to(F64)
    P3 = _row(Q[3], x, y, fd)
    usable = ok(d, v0[:, ::step, ::step]) & torch.isfinite(P3) & (P3 != 0) & torch.isfinite(w) & (w > 0)
    X = [_row(Q[i], x, y, fd) / P3 for i in range(3)]
    Y = [((Tb[:, 4 * i] * X[0] + Tb[:, 4 * i + 1] * X[1]) + Tb[:, 4 * i + 2] * X[2]) + Tb[:, 4 * i + 3] for i in range(3)]
    h = [_row(A[q], Y[0], Y[1], Y[2]) for q in range(4)]
    u, v, dn = h[0] / h[3], h[1] / h[3], h[2] / h[3]
    cand = usable & torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(dn) & (dn > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) \
        & (v <= H - 1)
    uc, vc = torch.where(cand, u, torch.zeros_like(u)), torch.where(cand, v, torch.zeros_like(v))
    x0, y0 = torch.floor(uc).clamp(max=W - 2).long(), torch.floor(vc).clamp(max=H - 2).long()
    fx, fy = u - x0.to(F64), v - y0.to(F64)
    bi = torch.arange(B).view(B, 1, 1).expand_as(x0)
    taps = [disp1[bi, y0 + dy, x0 + dx] for dy in (0, 1) for dx in (0, 1)]                       # d00 d01 d10 d11
    tv = [v1[bi, y0 + dy, x0 + dx] for dy in (0, 1) for dx in (0, 1)]
    taps_ok = ok(taps[0], tv[0]) & ok(taps[1], tv[1]) & ok(taps[2], tv[2]) & ok(taps[3], tv[3])
    st = torch.stack(taps)
    spread = st.max(0).values.to(F64) - st.min(0).values.to(F64)
    d00, d01, d10, d11 = (t.to(F64) for t in taps)
    top, bot = d00 + fx * (d01 - d00), d10 + fx * (d11 - d10)
    s = top + fy * (bot - top)
    gx = (1.0 - fy) * (d01 - d00) + fy * (d11 - d10)
    gy = (1.0 - fx) * (d10 - d00) + fx * (d11 - d01)
    r = s - dn
    used = cand & taps_ok & ~(spread > float(f32(tap_range))) & (r.abs() <= float(f32(max_residual)))
    dh = [[A[q, 0].expand_as(u), A[q, 1].expand_as(u), A[q, 2].expand_as(u), A[q, 2] * Y[1] - A[q, 1] * Y[2],
           A[q, 0] * Y[2] - A[q, 2] * Y[0], A[q, 1] * Y[0] - A[q, 0] * Y[1]] for q in range(4)]
    J = []
    for j in range(6):
        du, dv, dd = (dh[0][j] - u * dh[3][j]) / h[3], (dh[1][j] - v * dh[3][j]) / h[3], (dh[2][j] - dn * dh[3][j]) / h[3]
        J.append((gx * du + gy * dv) - dd)
    c = float(f32(cauchy))
    k = 1.0 / (1.0 + ((w * r) * r) / (c * c))
    a = k * w
    terms = [(a * J[j]) * J[i] for j in range(6) for i in range(j, 6)] + [(a * J[j]) * r for j in range(6)] + [(a * r) * r, a]
    zero = torch.zeros_like(u)
    terms = [torch.where(used, t, zero) for t in terms]
    n = used.sum((1, 2)).to(F64)
    sums = torch.zeros(B, 32, dtype=F64)
    bound = torch.zeros(B, 32, dtype=F64)
    for i, t in enumerate(terms):
        sums[:, i] = t.sum((1, 2))
        bound[:, i] = n * 2.0 ** -52 * t.abs().sum((1, 2))
    sums[:, 29], sums[:, 30] = n, cand.sum((1, 2)).to(F64)
    residual = torch.full((B, H, W), NAN, dtype=torch.float32)
    residual[:, ::step, ::step] = torch.where(used, r, torch.full_like(r, NAN)).to(torch.float32)
    return {"sums": sums, "bound": bound, "residual": residual, "used": used, "cand": cand, "r": r, "J": torch.stack(J, -1), "u": u,
            "v": v, "gx": gx, "gy": gy, "s": s, "dn": dn}


# ---- the scene the GPU test shares ------------------------------------------------------------------------------------------------------
PLANES = torch.tensor([[0.3, 0.1, 1.0, -3.0], [-0.4, 0.2, 1.0, -3.1], [0.05, -0.5, 1.0, -3.2]], dtype=F64)   # n . X + c = 0, metres
TRUE_MOTION = rigid(0.006, 0.015, -0.004, 0.05, -0.02, 0.06)              # about 1 degree and 8 cm


def scene_q(H, W):
    return ecm().ops.q_matrix(1.25 * W, 0.25, 0.5 * W - 0.3, 0.5 * H + 0.2)


def render(pose, H, W, planes=PLANES, Q=None):
    """The disparity map [H,W] (fp64) of the planes (given in the frame pose = I) seen from the frame that `pose` takes points
    into: a plane pi of that frame gives d = -(pi . Q[:, (0,1,3)] . (x,y,1)) / (pi . Q[:, 2]); a pixel takes the largest."""
    Q = scene_q(H, W) if Q is None else Q
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    xy1 = torch.stack([xs, ys, torch.ones_like(xs)])
    maps = []
    for pi in planes @ torch.linalg.inv(pose):
        pq = pi @ Q
        maps.append(-(pq[0] * xy1[0] + pq[1] * xy1[1] + pq[3] * xy1[2]) / pq[2])
    return torch.stack(maps).max(0).values


def scene_pair(H=40, W=64, motion=TRUE_MOTION, planes=PLANES):
    """(disp0, disp1) [1,H,W] fp32 (each rounded once from the analytic map) and Q."""
    Q = scene_q(H, W)
    eye = torch.eye(4, dtype=F64)
    return (render(eye, H, W, planes, Q).to(torch.float32)[None], render(motion, H, W, planes, Q).to(torch.float32)[None], Q)


def pose_error(T, truth):
    return float(torch.linalg.vector_norm(ecm().ops.se3_log(T @ torch.linalg.inv(truth))))


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------
def test_the_identity_on_equal_maps_has_no_residual():
    d0, _, Q = scene_pair()
    res = align_t(d0, d0, Q, torch.eye(4, dtype=F64))
    # Q^-1 Q (x, y, d, 1) is (x, y, d, 1) to rounding: a border pixel may land an ulp outside the view, no interior one does
    assert bool(res["cand"][0, 1:-1, 1:-1].all()) and torch.equal(res["cand"], res["used"])
    assert float(res["r"][res["used"]].abs().max()) <= 40 * 2.0 ** -52 * float(d0.max())
    n = int(res["used"].sum())
    assert res["sums"][0, 29] == res["sums"][0, 30] == n >= 38 * 62 and res["sums"][0, 31] == 0
    assert bool(torch.isfinite(res["sums"]).all()) and float(res["sums"][0, 28]) == pytest.approx(n, rel=1e-12)


def test_the_true_motion_explains_the_second_map():
    d0, d1, Q = scene_pair()
    at_truth, at_rest = align_t(d0, d1, Q, TRUE_MOTION), align_t(d0, d1, Q, torch.eye(4, dtype=F64))
    rms = lambda s: math.sqrt(float(s["sums"][0, 27] / s["sums"][0, 28]))                        # noqa: E731
    assert int(at_truth["sums"][0, 29]) > 2000
    # bilinear sampling is exact on a planar facet: what is left is the fp32 rounding of the maps (2^-24 * 10 px) and the pixels
    # whose four taps straddle an edge between two facets
    assert rms(at_truth) < 0.02 * rms(at_rest) and float(at_truth["r"][at_truth["used"]].abs().median()) < 4e-6


def test_jacobian_against_central_differences():
    """J at a non-identity T against (r(exp(+e xi_j) T) - r(exp(-e xi_j) T)) / 2e on every pixel that all evaluations use.  Source
    pixels whose (u, v) lies within 1e-3 of an integer are masked out, and e is small enough (|du| <= 1.25 W * 4e-7) that no
    sample crosses a bilinear kink.  The tolerance is the quotient's own: rounding 3 E / e with
    E = 16 * 2^-52 * (|s| + |dn| + |gx| |u| + |gy| |v|) (r's evaluation error, 16 rounded operations deep, entering twice and once
    more through the estimate below), plus the truncation estimated by Richardson from a second quotient at 2e,
    |q(2e) - q(e)| (three times the leading term)."""
    ops = ecm().ops
    d0, d1, Q = scene_pair()
    T0 = rigid(0.004, 0.011, -0.002, 0.04, -0.015, 0.05)                   # near the truth, not at it, and not the identity
    base = align_t(d0, d1, Q, T0)
    near = lambda t: (t - torch.round(t)).abs() < 1e-3                                           # noqa: E731
    valid0 = (~(near(base["u"]) | near(base["v"])))[0][None]
    base = align_t(d0, d1, Q, T0, valid0=valid0)
    assert int(base["used"].sum()) > 2000
    e = 2e-7
    worst = 0.0
    for j in range(6):
        xi = torch.zeros(6, dtype=F64)
        q = []
        common = base["used"].clone()
        for scale in (1.0, 2.0):
            xi[j] = scale * e
            plus, minus = align_t(d0, d1, Q, ops.se3_exp(xi) @ T0, valid0=valid0), align_t(d0, d1, Q, ops.se3_exp(-xi) @ T0, valid0=valid0)
            common &= plus["used"] & minus["used"]
            q.append((plus["r"] - minus["r"]) / (2 * scale * e))
        assert int(common.sum()) > 0.95 * int(base["used"].sum())
        E = 16 * 2.0 ** -52 * (base["s"].abs() + base["dn"].abs() + base["gx"].abs() * base["u"].abs() + base["gy"].abs() * base["v"].abs())
        tol = 3 * E / e + (q[1] - q[0]).abs()
        err = (base["J"][..., j] - q[0]).abs()
        assert bool((err <= tol)[common].all()), (j, float((err - tol)[common].max()))
        assert float(tol[common].max()) < 1e-3 * float(base["J"][..., j][common].abs().max())    # the test can see a wrong J
        worst = max(worst, float(err[common].max()))
    print("jacobian: worst |J - quotient| =", worst)


def test_se3_exp_and_log():
    ops = ecm().ops
    eye = torch.eye(4, dtype=F64)
    assert torch.equal(ops.se3_exp(torch.zeros(6, dtype=F64)), eye)
    assert torch.equal(ops.se3_exp(torch.zeros(3, 6, dtype=F64)), eye.expand(3, 4, 4))
    assert torch.equal(ops.se3_log(eye), torch.zeros(6, dtype=F64))
    g = torch.Generator().manual_seed(5)
    axis = torch.randn(64, 3, generator=g, dtype=F64)
    axis = axis / torch.linalg.vector_norm(axis, dim=1, keepdim=True)
    angle = torch.cat([torch.tensor([1e-12, 1e-6, 0.0999, 0.1, 0.1001, 1.0, 3.0, 3.1], dtype=F64), 3.1 * torch.rand(56, generator=g, dtype=F64)])
    xi = torch.cat([torch.randn(64, 3, generator=g, dtype=F64), axis * angle[:, None]], 1)
    T = ops.se3_exp(xi)
    R = T[:, :3, :3]
    assert float((R @ R.transpose(1, 2) - eye[:3, :3]).abs().max()) < 1e-14 and float((torch.linalg.det(R) - 1).abs().max()) < 1e-14
    assert torch.equal(T[:, 3], eye[3].expand(64, 4))
    # against the matrix exponential of the 4x4 twist matrix
    X = torch.zeros(64, 4, 4, dtype=F64)
    X[:, :3, :3], X[:, :3, 3] = ops._hat(xi[:, 3:]), xi[:, :3]
    assert float((T - torch.linalg.matrix_exp(X)).abs().max()) < 1e-13
    # log(exp(xi)) == xi: the rotation vector is recovered from sin(angle), whose condition number is 1 / cos near pi/2 .. and
    # 1 / (pi - angle) near pi: 2^-52 * 4 / (pi - 3.1) = 2e-14 at the largest angle here; 1e-12 leaves two digits
    back = ops.se3_log(T)
    assert float((back - xi).abs().max()) < 1e-12, float((back - xi).abs().max())
    assert torch.equal(ops.se3_log(T[5]), back[5]) and torch.equal(ops.se3_exp(xi[5]), T[5])     # a single one is the batch's row
    # exp(a) exp(b) = exp(a + b) on one axis
    a = torch.tensor([0.1, -0.2, 0.3, 0.02, 0.01, -0.03], dtype=F64)
    assert float((ops.se3_exp(a) @ ops.se3_exp(2 * a) - ops.se3_exp(3 * a)).abs().max()) < 1e-15
    for bad in (torch.zeros(5, dtype=F64), torch.zeros(6), "xi", torch.full((6,), NAN, dtype=F64)):
        with pytest.raises(ValueError, match="se3_exp: xi"):
            ops.se3_exp(bad)
    with pytest.raises(ValueError, match="se3_log: T"):
        ops.se3_log(torch.eye(3, dtype=F64))


# ---- the closed loop: ops.motion_estimate's own loop over the restatement ---------------------------------------------------------------
def restated(d0, d1, Q, **kw):
    return lambda T: align_t(d0, d1, Q, T, **kw)["sums"]


def test_closed_loop_recovers_the_motion():
    ops = ecm().ops
    d0, d1, Q = scene_pair()
    est = ops.motion_estimate(d0, d1, Q, normal=restated(d0, d1, Q))
    err = pose_error(est.T[0], TRUE_MOTION)
    print("closed loop: pose error", err, "iterations", int(est.iterations[0]), "rms", float(est.rms[0]), "used", int(est.used[0]))
    assert isinstance(est, ops.MotionEstimate) and est._fields == ("T", "converged", "iterations", "used", "candidates", "rms", "information")
    assert est.T.shape == (1, 4, 4) and est.T.dtype == F64 and not est.T.is_cuda
    assert bool(est.converged[0]) and int(est.iterations[0]) <= 10 and int(est.used[0]) > 2000 and est.candidates[0] >= est.used[0]
    assert err <= MEASURED_POSE_ERROR, err                                # the restatement's own error: what POSE_BOUND is ten times
    assert torch.equal(est.T[0, 3], torch.tensor([0, 0, 0, 1], dtype=F64))
    ops.warp_matrix(Q, est.T)                                              # the form DisparityTracker takes as `motion`
    assert est.information.shape == (1, 6, 6) and torch.equal(est.information, est.information.transpose(1, 2))
    # the three planes observe all six directions: the Jacobi-scaled information is well conditioned
    assert scaled_eigenvalues(est.information[0])[0] > 1e-4
    # from a per-image init, two images at once, each as alone
    two = ops.motion_estimate(torch.cat([d0, d0]), None, Q, init=torch.stack([torch.eye(4, dtype=F64), TRUE_MOTION]),
                              normal=restated(torch.cat([d0, d0]), torch.cat([d1, d1]), Q))
    assert torch.equal(two.T[0], est.T[0]) and bool(two.converged.all()) and two.iterations[1] < two.iterations[0]


def scaled_eigenvalues(H):
    s = torch.sqrt(torch.diagonal(H))
    return torch.linalg.eigvalsh(H / torch.outer(s, s))


def test_a_single_plane_is_reported_as_ill_conditioned():
    """A plane in (x, y, d) is mapped onto itself by three of the six motions (two translations in the plane and the rotation
    about its normal): the scaled information must show three directions that carry nothing -- at most 1e-6 of the mean
    eigenvalue 1, where the three-plane scene's smallest is above 1e-4 -- whatever pose the damped loop returns."""
    ops = ecm().ops
    d0, d1, Q = scene_pair(planes=PLANES[:1])
    est = ops.motion_estimate(d0, d1, Q, normal=restated(d0, d1, Q))
    ev = scaled_eigenvalues(est.information[0])
    print("single plane: scaled eigenvalues", ev.tolist())
    assert bool((ev[:3] < 1e-6).all()) and bool((ev[3:] > 1e-3).all()), ev
    assert bool(torch.isfinite(est.T).all())


def test_nothing_to_align_returns_init():
    ops = ecm().ops
    d0, d1, Q = scene_pair()
    init = rigid(0.001, 0.002, 0.003, 0.01, 0.02, 0.03)
    nothing = torch.zeros_like(d0, dtype=torch.bool)
    for kw in ({"valid0": nothing}, {"valid1": nothing}, {"weight": torch.full_like(d0, NAN)}, {"max_disp": 0.5}):
        est = ops.motion_estimate(d0, d1, Q, init=init, normal=restated(d0, d1, Q, **kw))
        assert torch.equal(est.T[0], init) and not bool(est.converged[0]) and int(est.used[0]) == 0 and int(est.iterations[0]) == 0
        assert math.isnan(float(est.rms[0])) and bool(torch.isfinite(est.information).all())
    # fewer than min_pixels: a 5x5 window is 25 pixels
    window = nothing.clone()
    window[:, 10:15, 20:25] = True
    est = ops.motion_estimate(d0, d1, Q, init=init, normal=restated(d0, d1, Q, valid0=window))
    assert torch.equal(est.T[0], init) and not bool(est.converged[0]) and 0 < int(est.used[0]) < 64
    one = ops.motion_estimate(d0, d1, Q, init=init, iterations=1, normal=restated(d0, d1, Q))
    n = int(one.used[0])
    assert int(one.iterations[0]) == 1 and not torch.equal(one.T[0], init) and n > 2000
    for min_pixels, steps in ((n, 1), (n + 1, 0)):                         # the threshold itself
        est = ops.motion_estimate(d0, d1, Q, init=init, iterations=1, min_pixels=min_pixels, normal=restated(d0, d1, Q))
        assert int(est.iterations[0]) == steps and torch.equal(est.T[0], one.T[0] if steps else init) and int(est.used[0]) == n
    # sums that are not finite, and an image that fails beside one that does not
    both = ops.motion_estimate(torch.cat([d0, d0]), None, Q, init=init,
                               normal=lambda T: torch.cat([align_t(d0, d1, Q, T[:1])["sums"], torch.full((1, 32), NAN, dtype=F64)]))
    assert bool(both.converged[0]) and not bool(both.converged[1]) and torch.equal(both.T[1], init)
    assert pose_error(both.T[0], TRUE_MOTION) <= MEASURED_POSE_ERROR


def test_special_values_are_decided_as_stated():
    Q = scene_q(4, 6)
    # a sideways motion that keeps every depth: at d = 5 (b = 0.25) the pixel (x, y) lands on (x + 0.3, y + 0.3), so x0 = x and
    # y0 = y, and the last column and row leave the view: 5 x 3 candidates
    T = rigid(0, 0, 0, 0.015, 0.015, 0)
    d = torch.full((1, 4, 6), 5.0)
    count = lambda **kw: [int(v) for v in align_t(kw.pop("d0", d), kw.pop("d1", d), Q, T, **kw)["sums"][0, 29:31]]    # noqa: E731
    assert count() == [15, 15]
    for bad in (NAN, INF, -INF, 0.0, -1.0):
        d0 = d.clone()
        d0[0, 1, 2] = bad
        assert count(d0=d0) == [14, 14]                                    # an unusable source pixel is no candidate
        d1 = d.clone()
        d1[0, 1, 2] = bad
        assert count(d1=d1) == [11, 15]                                    # (1,2) is a tap of the four pixels up and left of it
    for bad in (NAN, INF, -INF, 0.0, -2.0):
        w = torch.ones(1, 4, 6)
        w[0, 0, 0] = bad
        assert count(weight=w) == [14, 14]
    edge = d.clone()
    edge[0, :, 3:] = 6.5                                                   # a depth edge between columns 2 and 3
    assert count(d0=edge, d1=edge) == [12, 15] and count(d0=edge, d1=edge, tap_range=2.0) == [15, 15]
    assert count(d0=edge, d1=edge, tap_range=2.0, max_residual=0.25) == [12, 15]                # r = 0.3 * 1.5 across the edge
    assert count(step=2) == [6, 6] and count(step=3) == [2, 2] and count(step=7) == [1, 1]
    assert count(min_disp=5.0) == [0, 0] and count(max_disp=5.0) == [15, 15]
    v = torch.ones(1, 4, 6, dtype=torch.uint8)
    v[0, 1, 2] = 0
    assert count(valid0=v) == [14, 14] and count(valid1=v) == [11, 15]
    # a Q of powers of two: the identity maps every pixel onto itself exactly, and the last column and row sample with fx, fy = 1
    Qp = ecm().ops.q_matrix(64.0, 0.25, 4.0, 2.0)
    d = torch.full((1, 4, 6), 4.0)
    res = align_t(d, d, Qp, torch.eye(4, dtype=F64))
    assert torch.equal(res["u"][0, 0], torch.arange(6, dtype=F64)) and torch.equal(res["v"][0, :, 0], torch.arange(4, dtype=F64))
    assert [int(s) for s in res["sums"][0, 29:31]] == [24, 24] and float(res["r"].abs().max()) == 0.0


# ---- the census of the fifth header -------------------------------------------------------------------------------------------------------
def header_prototypes():
    with open(os.path.join(INCLUDE, HEADER)) as f:
        return parse_header(f.read())


def test_the_registries():
    lib = ecm()._lib
    assert lib.REGISTRIES[0] is lib.TABLES and lib.REGISTRIES[1] is lib.EXTENSION_TABLES and len(lib.REGISTRIES) == 3
    assert tuple(lib.REGISTRIES[2]) == (HEADER,) and lib.REGISTRIES[2][HEADER][0] is lib.MOTION_PROTOTYPES
    assert lib.REGISTRIES[2][HEADER][1] == PREFIX
    rows = dict(lib._tables())
    assert all(n in rows for n in ENTRIES) and "ecm_abi_version" in rows and "ecmt_disparity_fuse_fwd" in rows
    assert len(rows) == sum(len(t) for reg in lib.REGISTRIES for t, _ in reg.values())          # no name in two tables


def test_header_table_and_package_literals_name_the_same_entries():
    import re
    lib = ecm()._lib
    parsed = header_prototypes()
    with open(os.path.join(INCLUDE, HEADER)) as f:
        by_text = set(re.findall(rf"\b({PREFIX}[a-z0-9_]+)\s*\(", _strip(f.read())))
    found = package_entry_names(PREFIX + "[a-z0-9_]+", "MOTION_PROTOTYPES")
    assert sorted(parsed) == sorted(by_text) == sorted(lib.MOTION_PROTOTYPES) == sorted(found) == sorted(ENTRIES)
    assert all(n.startswith(PREFIX) for n in parsed)
    assert all(a.startswith("ops.py:") for at in found.values() for a in at), found
    for registry in lib.REGISTRIES[:2]:
        for table, _ in registry.values():
            assert not set(table) & set(lib.MOTION_PROTOTYPES)


def test_prototypes_match_the_header_type_by_type():
    table, parsed = ecm()._lib.MOTION_PROTOTYPES, header_prototypes()
    assert compare(parsed, table) == []
    assert all(table[n] == parsed[n] for n in parsed)


def test_library_exports_every_row_and_load_types_it(lib_mod):
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(lib, n)] == [] and lib_mod.missing_symbols() == []
    table = lib_mod.MOTION_PROTOTYPES
    real = dict(table)
    try:
        table[PREFIX + "not_there"] = (C.c_int, [])
        assert lib_mod.missing_symbols() == [PREFIX + "not_there"]
    finally:
        table.clear()
        table.update(real)
    loaded = lib_mod.load()
    for name, (res, args) in table.items():
        assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == args, name
    assert ecm().ops.ALIGN_SUMS == ecm().ops.align_sums() == lib_mod.query("ecmm_align_sums") == 32


def tiles(H, W, step):
    return -(-(-(-H // step) * -(-W // step)) // TILE)


def test_size_query_against_the_tile_count(lib_mod):
    for B in (1, 3, 64):
        for H in (2, 3, 37, 40, 576, 4097):
            for W in (2, 61, 64, 960, 2049):
                for step in (1, 2, 3, 7, 5000):
                    assert lib_mod.query("ecmm_align_scratch_bytes", B, H, W, step) == B * tiles(H, W, step) * 32 * 8, (B, H, W, step)
    assert [tiles(*s) for s in ((2, 2, 1), (112, 128, 1), (128, 128, 1), (129, 128, 1), (263, 256, 1), (37, 61, 1))] == [1, 7, 8, 9, 33, 2]
    for refused in ((0, 4, 4, 1), (1, 1, 4, 1), (1, 4, 1, 1), (1, 4, 4, 0), (1, 4, 4, -1), (1, 65536, 32768, 1), (1, 65536, 32768, 64),
                    (65536, 4096, 4096, 1)):
        assert lib_mod.query("ecmm_align_scratch_bytes", *refused) == 0, refused
    assert lib_mod.query("ecmm_align_scratch_bytes", 65536, 4096, 4096, 4) == 0
    assert lib_mod.query("ecmm_align_scratch_bytes", 65536, 4096, 4096, 8) == 65536 * 128 * 256        # the lattice is what is tiled


# ---- the refusal contract, with the devices hidden --------------------------------------------------------------------------------------
ROWS = [
    Row("ecmm_align_normal_fwd",
        "disp0:p valid0:o weight0:o disp1:p valid1:o Q:p Qinv_out:p T:p t_per_image=~0 sums:p residual:o scratch:p scratch_bytes=Q0 "
        "B=1 H=2 W=2 step=1 min_disp=f0 max_disp=f100 tap_range=f1 max_residual=f3 cauchy=f1 stream:s",
        queries=[("ecmm_align_scratch_bytes", "B H W step")],
        inval=[{"H": 1}, {"W": 1}], legal=[{"t_per_image": 1}, {"step": 5}],
        # "H * W >= 2^31, or B * ceil(ceil(H / step) * ceil(W / step) / 2048) >= 2^24"
        unsup=[{"H": 65536, "W": 32768}, {"B": 65536, "H": 4096, "W": 4096}], header=HEADER),
]
QUERIES = [Row("ecmm_align_scratch_bytes", "B=1 H=2 W=2 step=1", header=HEADER)]
INT_CONSTS = ("ecmm_align_sums",)


@pytest.fixture(scope="module")
def results(lib_mod):
    """{call id: return value} of the rows above from one fresh child that sees no device (tests/abi_refusal_child.py)."""
    parsed = header_prototypes()
    calls = [{"id": f"const|{n}", "fn": n, "res": "i", "args": []} for n in INT_CONSTS]
    for row in ROWS:
        calls += calls_of(row, lambda q: parsed[q][1])
    for row in QUERIES:
        calls += query_calls(row)
    assert len({c["id"] for c in calls}) == len(calls)
    env = dict(os.environ)
    env.update(HIDE)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__)], input=json.dumps({"lib": lib_mod.LIB_PATH, "calls": calls}),
                       capture_output=True, text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    seen = next((ln.split()[1] for ln in lines if ln.startswith("DEVICES ")), None)
    assert seen is not None and seen.isdigit(), f"the child did not report a device count (exit {r.returncode}): {r.stderr[-2000:]}"
    if seen != "0":
        pytest.skip(f"the child sees {seen} device(s) although {sorted(HIDE)} hide them: no ABI call was made")
    got = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("R ")}
    if "DONE" not in lines:
        nxt = next((c["id"] for c in calls if c["id"] not in got), None)
        pytest.fail(f"the child ended with status {r.returncode} in call {nxt}: {r.stderr[-2000:]}")
    return got


def test_every_entry_of_the_fifth_header_has_a_row():
    parsed = header_prototypes()
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    assert sorted(ent) == sorted(r.name for r in ROWS) and sorted(qry) == sorted(r.name for r in QUERIES)
    for r in ROWS + QUERIES:
        assert r.types == (ent.get(r.name) or qry[r.name]), r.name
    assert sorted(set(parsed) - set(ent) - set(qry)) == sorted(INT_CONSTS)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    row = next(r for r in ROWS if r.name == name)
    bad = classify(row, results)
    assert not bad, "\n" + _report(bad)
    assert results[f"{name}|accepted"] > 0                                 # the pointers are never dereferenced: no device, no crash


def test_size_query_is_zero_for_sizes_it_cannot_serve(results):
    row = QUERIES[0]
    bad = classify_query(row, results)
    assert not bad, "\n" + _report(bad)
    assert results["ecmm_align_normal_fwd|query0@H=65536,W=32768"] == 0 and results["ecmm_align_normal_fwd|query0@H=1"] == 0
    assert results["ecmm_align_normal_fwd|query0@step=0"] == 0


def test_further_refusals_of_the_entry(lib_mod):
    """What the row cannot express: floats, and an output that is an input or another output.  Every call returns before any HIP
    call."""
    lib = lib_mod.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(12)]                    # never dereferenced
    names = ("disp0", "valid0", "weight0", "disp1", "valid1", "Q", "Qinv_out", "T")
    base = [(n, p[i]) for i, n in enumerate(names)] + [
        ("per", 0), ("sums", p[8]), ("residual", p[9]), ("scratch", p[10]), ("bytes", 256), ("B", 1), ("H", 2), ("W", 2), ("step", 1),
        ("lo", 0.0), ("hi", 100.0), ("tap_range", 1.0), ("max_residual", 3.0), ("cauchy", 1.0), ("stream", None)]
    call = lambda **kw: lib.ecmm_align_normal_fwd(*[kw.get(k, v) for k, v in base])              # noqa: E731
    for out in ("sums", "residual", "scratch"):
        for i, n in enumerate(names):
            assert call(**{out: p[i]}) == EINVAL, (out, n)
    assert call(residual=p[8]) == EINVAL and call(scratch=p[8]) == EINVAL and call(scratch=p[9]) == EINVAL
    for kw in ({"lo": NAN}, {"lo": INF}, {"hi": NAN}, {"lo": 2.0, "hi": 1.0}):
        assert call(**kw) == EINVAL, kw
    for name in ("tap_range", "max_residual", "cauchy"):
        for bad in (0.0, -1.0, NAN, INF):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    assert call(bytes=255) == ESCRATCH and call(B=2, bytes=511) == ESCRATCH and call(H=65536, W=32768) == EUNSUP
    # no legal call is made here: this process may see a device, and the pointers are not device memory (the child's rows make
    # the accepted call, with the devices hidden)


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
class OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the shape and dtype contract is checked before anything is launched."""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


def test_op_signatures():
    ops = ecm().ops
    sig = inspect.signature(ops.motion_normal)
    assert list(sig.parameters) == ["disp0", "disp1", "Q", "T", "valid0", "valid1", "weight", "Q_out", "step", "min_disp", "max_disp",
                                    "tap_range", "max_residual", "cauchy", "with_residual"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [None, None, None, None, 1, 0.0, None, 1.0, 3.0, 1.0, False]
    sig = inspect.signature(ops.motion_estimate)
    assert list(sig.parameters) == ["disp0", "disp1", "Q", "init", "valid0", "valid1", "weight", "Q_out", "step", "min_disp", "max_disp",
                                    "tap_range", "max_residual", "cauchy", "iterations", "damping", "tolerance", "min_pixels", "normal"]
    assert [p.default for p in list(sig.parameters.values())[14:]] == [10, 1e-6, 1e-7, 64, None]


def test_motion_normal_refusals():
    ops = ecm().ops
    eye = torch.eye(4, dtype=F64)
    Q = scene_q(4, 8)
    z = fake(1, 4, 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.motion_normal(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), Q, eye)
    for kw, match in (({"step": 0}, "step"), ({"step": 1.5}, "step"), ({"min_disp": NAN}, "min_disp"), ({"min_disp": 2.0, "max_disp": 1.0}, "max_disp"),
                      ({"tap_range": 0.0}, "tap_range"), ({"max_residual": -1.0}, "max_residual"), ({"cauchy": INF}, "cauchy"),
                      ({"cauchy": True}, "cauchy"), ({"Q_out": torch.zeros(4, 4, dtype=F64)}, "singular"), ({"Q_out": eye.float()}, "Q_out")):
        with pytest.raises(ValueError, match=match):
            ops.motion_normal(z, z, Q, eye, **kw)
    for bad in (Q.float(), torch.eye(3, dtype=F64), "Q", torch.full((4, 4), NAN, dtype=F64), torch.stack([Q, Q])):
        with pytest.raises(ValueError, match="motion_normal: Q"):
            ops.motion_normal(z, z, bad, eye)
    for bad in (eye.float(), torch.eye(3, dtype=F64), None, torch.full((4, 4), INF, dtype=F64)):
        with pytest.raises(ValueError, match="motion_normal: T"):
            ops.motion_normal(z, z, Q, bad)
    with pytest.raises(ValueError, match="one matrix, or one per image"):
        ops.motion_normal(fake(2, 4, 8), fake(2, 4, 8), Q, torch.stack([eye] * 3))
    for bad in (fake(4, 8), fake(1, 2, 4, 8), fake(1, 0, 8), fake(1, 1, 8), fake(1, 4, 1)):
        with pytest.raises(RuntimeError, match="motion_normal"):
            ops.motion_normal(bad, bad, Q, eye)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.motion_normal(fake(1, 4, 8, dtype=F64), z, Q, eye)
    for kw, match in (({"valid0": z}, "valid"), ({"valid1": fake(1, 4, 9, dtype=torch.bool)}, "valid"), ({"weight": fake(1, 4, 8, dtype=F64)}, "weight"),
                      ({"weight": fake(1, 5, 8)}, "weight")):
        with pytest.raises(RuntimeError, match=match):
            ops.motion_normal(z, z, Q, eye, **kw)
    with pytest.raises(RuntimeError, match="disp1"):
        ops.motion_normal(z, fake(1, 4, 9), Q, eye)
    assert ops.check_align_parameters(2, 1, None, 0.5, 2, 3) == (2, 1.0, FLT_MAX, 0.5, 2.0, 3.0)


def test_motion_estimate_refusals():
    ops = ecm().ops
    d0, d1, Q = scene_pair()
    for kw, match in (({"iterations": 0}, "iterations"), ({"iterations": 2.5}, "iterations"), ({"damping": -1.0}, "damping"),
                      ({"tolerance": NAN}, "tolerance"), ({"min_pixels": 0}, "min_pixels"), ({"step": 0}, "step"), ({"cauchy": 0}, "cauchy"),
                      ({"init": torch.eye(4)}, "init"), ({"init": torch.stack([torch.eye(4, dtype=F64)] * 2)}, "init")):
        with pytest.raises(ValueError, match="motion_estimate: " + match):
            ops.motion_estimate(d0, d1, Q, normal=restated(d0, d1, Q), **kw)
    with pytest.raises(RuntimeError, match="CPU tensor"):                  # without `normal` it is the device op
        ops.motion_estimate(d0, d1, Q)


def test_odometry_refusals_and_the_split_tracker():
    e = ecm()
    models, ops = e.models, e.ops
    net, Q = e.get_model("cmfsm"), ops.q_matrix(700.0, 0.25, 64.0, 32.0)
    sig = inspect.signature(models.StereoOdometry.__init__)
    assert list(sig.parameters) == ["self", "model", "Q", "head", "step", "iterations", "damping", "tolerance", "min_pixels", "tap_range",
                                    "max_residual", "cauchy", "gate", "process_noise", "sigma0", "footprint", "coast"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [2, 2, 10, 1e-6, 1e-7, 64, 1.0, 3.0, 1.0, 3.0, 0.01, 1.0, "cover", True]
    assert models.Odometry._fields == models.Tracked._fields + ("motion", "pose", "estimate", "restarted")
    for kw, match in (({"head": 3}, "head"), ({"step": 0}, "step"), ({"iterations": 0}, "iterations"), ({"damping": NAN}, "damping"),
                      ({"min_pixels": 0.5}, "min_pixels"), ({"tap_range": 0}, "tap_range"), ({"cauchy": -1}, "cauchy"),
                      ({"gate": -1}, "gate"), ({"footprint": "both"}, "footprint")):
        with pytest.raises(ValueError, match=match):
            models.StereoOdometry(net, Q, **kw)
    with pytest.raises(ValueError, match="model"):
        models.StereoOdometry(torch.nn.Identity(), Q)
    for bad in (Q.float(), torch.zeros(4, 4, dtype=F64), torch.stack([Q, Q])):
        with pytest.raises(ValueError):
            models.StereoOdometry(net, bad)
    odo = models.StereoOdometry(net, Q)
    assert not isinstance(odo, torch.nn.Module) and isinstance(odo.tracker, models.DisparityTracker)
    x = torch.zeros(1, 3, 64, 128)                                         # CPU tensors: a forward on them raises RuntimeError
    with pytest.raises(RuntimeError):
        odo(x, x)
    odo.reset()
    assert odo.tracker._state is None and odo._pose is None and odo._velocity is None
    for half in ("measure", "carries", "advance"):
        assert callable(getattr(models.DisparityTracker, half))
