"""The TSDF volume without a GPU: integrate_t and raycast_t, fp64 torch restatements of
include/ecm_volume.h written from the header's text; every decision of the two definitions on hand-made volumes; the closed loop
(four analytic views of the three-plane scene integrated, a fifth raycast) on the restatements; ops.volume_matrices; the sixth
header's census and refusal contract; and models.StereoMapper's refusals and pose bookkeeping.
tests/test_hip_disp_volume.py compares the device with the two restatements.

Every operation of the restatements is one torch operation in the header's order (separate elementwise calls: nothing is fused),
so every value is the header's bit for bit."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import abi_refusal_child as child
from test_abi_refusals import EINVAL, EUNSUP, HIDE, Row, _report, calls_of, classify
from test_abi_types import INCLUDE, _strip, compare, lib_mod, package_entry_names, parse_header  # noqa: F401  (lib_mod: a fixture)
from test_disp_warp_cpu import rigid
from test_motion_align_cpu import PLANES, OnDevice, fake, render, scene_q

HEADER = "ecm_volume.h"
PREFIX = "ecmv_"
ENTRIES = ("ecmv_integrate_fwd", "ecmv_raycast_fwd", "ecmv_raycast_max_steps")
NAN, INF = float("nan"), float("inf")
FLT_MAX = 3.4028234663852886e38
F64, F32 = torch.float64, torch.float32
MAX_STEPS = 65536

# The mean absolute disparity error (pixels) of the closed loop below over the pixels that hit, for the restatement: set by the
# discretisation (0.06 m voxels seen at 3 m through 80 px of focal length, nearest-pixel lookups, creases between facets), not by
# rounding.  The device, whose per-voxel and per-pixel arithmetic is the restatement's, is held to ten times it, as POSE_BOUND is.
MEASURED_RAYCAST_ERROR = 2.6e-3
RAYCAST_BOUND = 10 * MEASURED_RAYCAST_ERROR
HIT_SHARE = 0.8


def ecm():
    import ecm_amd
    return ecm_amd


def f32(v):
    return torch.tensor(v, dtype=F32)


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def _row(m, a, b, c):
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3]


def _view(M, v):
    return M[v] if M.dim() == 3 else M


def integrate_t(tsdf, wsum, disp, Q, G, Cm, trunc, valid=None, weight=None, max_weight=64.0, min_disp=0.0, max_disp=None, seen=None):
    """include/ecm_volume.h's integration on CPU tensors: (tsdf, wsum, touched), new tensors; touched: some view updated the voxel.
    After the tsdf step of view v, seen(v, ok, (yi, xi), w, s) is called with the voxels the view updated, the pixel each voxel
    reads, its weight and s = z_meas - z_vox (include/ecm_color.h's attribute step hangs there); it changes nothing here."""
    nz, ny, nx = tsdf.shape
    V, H, W = disp.shape
    lo, hi = f32(min_disp), f32(FLT_MAX if max_disp is None else min(max_disp, FLT_MAX))
    tr, mw = float(f32(trunc)), f32(max_weight)
    kk, jj, ii = (t.to(F64) for t in torch.meshgrid(torch.arange(nz), torch.arange(ny), torch.arange(nx), indexing="ij"))
    X, N = tsdf.clone(), wsum.clone()
    touched = torch.zeros(nz, ny, nx, dtype=torch.bool)
    zero = torch.zeros_like(ii)
    for v in range(V):
        Gv, Cv = _view(G, v), _view(Cm, v)
        h = [_row(Gv[r], ii, jj, kk) for r in range(4)]
        u, vv, dv = h[0] / h[3], h[1] / h[3], h[2] / h[3]
        ok = torch.isfinite(u) & torch.isfinite(vv) & torch.isfinite(dv) & (dv > 0)
        px, py = torch.floor(u + 0.5), torch.floor(vv + 0.5)
        ok = ok & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        px, py = torch.where(ok, px, zero), torch.where(ok, py, zero)
        xi, yi = px.long(), py.long()
        d = disp[v][yi, xi]
        val = torch.ones_like(ok) if valid is None else valid[v][yi, xi] != 0
        w = torch.ones_like(d) if weight is None else weight[v][yi, xi]
        ok = ok & torch.isfinite(d) & val & (d > lo) & (d <= hi) & torch.isfinite(w) & (w > 0)
        fd = d.to(F64)
        P3 = _row(Q[3], px, py, fd)
        ok = ok & torch.isfinite(P3) & (P3 != 0)
        z_meas = _row(Q[2], px, py, fd) / P3
        z_vox = _row(Cv[2], ii, jj, kk)
        ok = ok & torch.isfinite(z_meas) & (z_meas > 0) & torch.isfinite(z_vox) & (z_vox > 0)
        s = z_meas - z_vox
        ok = ok & ~(s < -tr)
        t = torch.clamp(s / tr, max=1.0).to(F32)
        Wn = N + w
        Xn = (X * N + t * w) / Wn
        Nn = torch.minimum(Wn, mw)
        X, N = torch.where(ok, Xn, X), torch.where(ok, Nn, N)
        touched |= ok
        if seen is not None:
            seen(v, ok, (yi, xi), w, s)
    return X, N, touched


def _blend(plane, cell, q):
    x, y, z = cell
    t = lambda dz, dy, dx: plane[z + dz, y + dy, x + dx].to(F64)                                 # noqa: E731
    a = [[t(dz, dy, 0) + q[0] * (t(dz, dy, 1) - t(dz, dy, 0)) for dy in (0, 1)] for dz in (0, 1)]
    e = [a[dz][0] + q[1] * (a[dz][1] - a[dz][0]) for dz in (0, 1)]
    return e[0] + q[2] * (e[1] - e[0])


def raycast_t(tsdf, wsum, R, Rinv, size, near_disp, far_disp, step=0.5, max_steps=MAX_STEPS, at_hit=None):
    """include/ecm_volume.h's raycast on CPU tensors: a dict of out and hit_weight [B,H,W] fp32, hit (bool) and n (fp64).  Where
    rays of view b hit, at_hit(b, hit, cell, q) is called with the mask, the clamped cell about each crossing ([x, y, z], long; 0
    off the mask) and the crossing's position within it, the operands of hit_weight's blend (include/ecm_color.h's blend of the
    attributes hangs there); it changes nothing here."""
    nz, ny, nx = tsdf.shape
    dims = (nx, ny, nz)
    H, W = size
    Rb, Rib = (R, Rinv) if R.dim() == 3 else (R[None], Rinv[None])
    near, far, st = float(f32(near_disp)), float(f32(far_disp)), float(f32(step))
    ys, xs = (t.to(F64) for t in torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij"))
    zero = torch.zeros_like(xs)
    outs, weights, hits, ns = [], [], [], []
    for b, (Rm, Ri) in enumerate(zip(Rb, Rib)):
        hn, hf = [_row(Rm[r], xs, ys, near) for r in range(4)], [_row(Rm[r], xs, ys, far) for r in range(4)]
        gn, gf = [hn[a] / hn[3] for a in range(3)], [hf[a] / hf[3] for a in range(3)]
        dr = [gf[a] - gn[a] for a in range(3)]
        ln = torch.sqrt((dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2])
        nd = torch.ceil(ln / st)
        live = (nd >= 1) & (nd <= max_steps)
        for t in gn + gf:
            live = live & torch.isfinite(t)
        ndc = torch.where(live, nd, torch.ones_like(nd))
        done = ~live
        before = torch.zeros_like(live)
        f0, p0 = zero, [zero, zero, zero]
        res, hw, hit_any = torch.zeros(H, W, dtype=F32), torch.zeros(H, W, dtype=F32), torch.zeros_like(live)
        for m in range(int(ndc.max()) + 1):
            act = ~done & (m <= ndc)
            if not bool(act.any()):
                break
            s = m / ndc
            p = [gn[a] + dr[a] * s for a in range(3)]
            c = [torch.floor(p[a]) for a in range(3)]
            ok = act
            for a in range(3):
                ok = ok & (c[a] >= 0) & (c[a] <= dims[a] - 2)
            cell = [torch.where(ok, c[a], zero).long() for a in range(3)]
            q = [p[a] - c[a] for a in range(3)]
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        ok = ok & (wsum[cell[2] + dz, cell[1] + dy, cell[0] + dx] > 0)
            f = _blend(tsdf, cell, q)
            pair = ok & before
            hit = pair & (f0 > 0) & (f <= 0)
            back = pair & (f0 < 0) & (f > 0)
            al = f0 / (f0 - f)
            ps = [p0[a] + (p[a] - p0[a]) * al for a in range(3)]
            val = (_row(Ri[2], ps[0], ps[1], ps[2]) / _row(Ri[3], ps[0], ps[1], ps[2])).to(F32)
            res = torch.where(hit, val, res)
            wc = [torch.where(hit, torch.floor(ps[a]).clamp(0, dims[a] - 2), zero) for a in range(3)]
            at, within = [t.long() for t in wc], [ps[a] - wc[a] for a in range(3)]
            hw = torch.where(hit, _blend(wsum, at, within).to(F32), hw)
            if at_hit is not None and bool(hit.any()):
                at_hit(b, hit, at, within)
            hit_any |= hit
            done = done | hit | back
            before, f0, p0 = ok, f, p
        outs.append(res), weights.append(hw), hits.append(hit_any), ns.append(nd)
    return {"out": torch.stack(outs), "hit_weight": torch.stack(weights), "hit": torch.stack(hits), "n": torch.stack(ns)}


# ---- the scene the GPU test shares ------------------------------------------------------------------------------------------------------
H0, W0 = 40, 64
DIMS = (48, 48, 48)
VOXEL, ORIGIN, TRUNC = 0.06, (-1.44, -1.44, 1.7), 0.25      # x, y in +-1.44 m, z in 1.7 .. 4.58 m: the planes lie at about 3 m
NEAR, FAR = 12.0, 4.0                                        # disparities: 1.67 m and 5 m
VIEWS = [torch.eye(4, dtype=F64), rigid(0.006, 0.015, -0.004, 0.05, -0.02, 0.06), rigid(-0.01, 0.02, 0.0, -0.06, 0.03, -0.04),
         rigid(0.012, -0.018, 0.006, 0.08, 0.04, 0.02)]
FIFTH = rigid(0.004, 0.008, -0.003, 0.02, 0.01, 0.03)


def scene_views(poses=VIEWS):
    """(disp [V,H0,W0] fp32, each view rounded once from the analytic map, and Q)."""
    Q = scene_q(H0, W0)
    return torch.stack([render(p, H0, W0, PLANES, Q).to(F32) for p in poses]), Q


def empty(dims):
    return torch.ones(dims, dtype=F32), torch.zeros(dims, dtype=F32)


_LOOP = {}


def closed_loop():
    """The restatement's closed loop, computed once: the integrated volume, the raycast at FIFTH and the analytic map there."""
    if not _LOOP:
        ops = ecm().ops
        disp, Q = scene_views()
        m = ops.volume_matrices(Q, torch.stack(VIEWS), ORIGIN, VOXEL)
        tsdf, wsum, touched = integrate_t(*empty(DIMS), disp, Q, m.G, m.C, TRUNC)
        r = ops.volume_matrices(Q, FIFTH, ORIGIN, VOXEL)
        cast = raycast_t(tsdf, wsum, r.R, r.Rinv, (H0, W0), NEAR, FAR)
        _LOOP.update(tsdf=tsdf, wsum=wsum, touched=touched, cast=cast, truth=render(FIFTH, H0, W0, PLANES, Q), Q=Q, disp=disp)
    return _LOOP


def loop_error(out, truth):
    """(share of the pixels that hit, mean |out - truth| over them)."""
    hit = out > 0
    return float(hit.to(F64).mean()), float((out.to(F64) - truth)[hit].abs().mean())


def test_closed_loop_of_the_restatement():
    loop = closed_loop()
    share, err = loop_error(loop["cast"]["out"][0], loop["truth"])
    print("closed loop: hit share", share, "mean |d - truth|", err, "touched voxels", int(loop["touched"].sum()),
          "largest n", float(loop["cast"]["n"].max()))
    assert bool((loop["truth"] > FAR).all()) and bool((loop["truth"] < NEAR).all())              # every pixel sees a plane in range
    assert torch.equal(loop["cast"]["hit"][0], loop["cast"]["out"][0] > 0)
    assert share >= HIT_SHARE, share
    assert err <= MEASURED_RAYCAST_ERROR, err                             # the restatement's own error: what RAYCAST_BOUND is ten times
    assert bool(((loop["tsdf"] >= -1) & (loop["tsdf"] <= 1)).all()) and bool((loop["wsum"] <= 4).all())
    assert torch.equal(loop["wsum"] > 0, loop["touched"])
    hw = loop["cast"]["hit_weight"][0]
    assert bool((hw[loop["cast"]["hit"][0]] > 0).all()) and bool((hw[~loop["cast"]["hit"][0]] == 0).all())


# ---- the mapper's closed loop ------------------------------------------------------------------------------------
# models.StereoMapper composes three conventions that no other test composes: world = motion @ world, T is world to camera, and
# the frame's OWN disparity (not the fused state) goes into the volume.  The reference loop below states them on the restatements:
# five analytic views of the three-plane scene along a constant screw motion, each frame's motion estimated by
# ops.motion_estimate's own host loop over align_t from the previous frame's map to this one (the device aligns the tracker's
# fused state, which on an analytic scene is the previous map carried and averaged), the pose composed as the class documents it,
# the frame's map integrated with the mapper's valid = d > 0 and weight = 1 / std^2, and the volume raycast at a pose that none
# of the five views has.
MAPPER_STEP = rigid(0.003, 0.007, -0.002, 0.025, -0.01, 0.03)              # step1 of test_stereo_odometry_is_the_tracker_fed_the_estimate
MAPPER_STD = 0.05
MAPPER_MIN_DISP = 1.0                                                       # StereoMapper's default
MAPPER_HELD_OUT = rigid(0.005, -0.006, 0.004, -0.04, 0.03, 0.05)           # off the path: no view was taken here


def mapper_poses(n=5):
    """I, s, s^2, ...: the world-to-camera pose of frame k (the world frame is frame 0's left camera)."""
    poses = [torch.eye(4, dtype=F64)]
    for _ in range(n - 1):
        poses.append(MAPPER_STEP @ poses[-1])
    return poses


def mapper_maps(poses=None):
    """(maps [5,H0,W0] fp32, each rounded once from the analytic map, and Q)."""
    return scene_views(mapper_poses() if poses is None else poses)


# Both measured on the CPU with the restatements (the loop below prints them): the mean absolute disparity error over the pixels
# that hit, in pixels, and the share of the pixels that hit.  The error is set by the discretisation (RAYCAST's, above) and by the
# accumulated pose error of four estimates, not by rounding; the device's StereoMapper is held to ten times it.
MEASURED_MAPPER_ERROR = 3.7e-3                                             # 3.687e-3 as printed
MEASURED_MAPPER_HIT_SHARE = 0.88                                           # 0.8863 as printed
MAPPER_BOUND = 10 * MEASURED_MAPPER_ERROR
_MAPPER_LOOP = {}


def mapper_loop():
    """The reference loop, computed once: the world poses, the volume, the raycast at MAPPER_HELD_OUT and the analytic map there."""
    if not _MAPPER_LOOP:
        from test_motion_align_cpu import restated
        ops = ecm().ops
        maps, Q = mapper_maps()
        world, worlds = torch.eye(4, dtype=F64), []
        tsdf, wsum = empty(DIMS)
        std = torch.full((1, H0, W0), MAPPER_STD, dtype=F32)
        velocity = None
        for k in range(maps.shape[0]):
            if k:
                est = ops.motion_estimate(maps[k - 1:k], maps[k:k + 1], Q, velocity, normal=restated(maps[k - 1:k], maps[k:k + 1], Q))
                assert bool(est.converged.all()), k
                velocity = est.T
                world = est.T[0] @ world                                   # world = motion @ world
            m = ops.volume_matrices(Q, world, ORIGIN, VOXEL)                # T is world to camera
            tsdf, wsum, _ = integrate_t(tsdf, wsum, maps[k:k + 1], Q, m.G, m.C, TRUNC, maps[k:k + 1] > 0, 1.0 / (std * std),
                                        min_disp=MAPPER_MIN_DISP)            # the frame's own map
            worlds.append(world.clone())
        r = ops.volume_matrices(Q, MAPPER_HELD_OUT, ORIGIN, VOXEL)
        cast = raycast_t(tsdf, wsum, r.R, r.Rinv, (H0, W0), NEAR, FAR)
        _MAPPER_LOOP.update(worlds=worlds, tsdf=tsdf, wsum=wsum, cast=cast, truth=render(MAPPER_HELD_OUT, H0, W0, PLANES, Q), Q=Q, maps=maps)
    return _MAPPER_LOOP


def test_mapper_loop_of_the_restatements():
    from test_motion_align_cpu import POSE_BOUND, pose_error
    loop = mapper_loop()
    poses = mapper_poses()
    errors = [pose_error(w, p) for w, p in zip(loop["worlds"], poses)]
    share, err = loop_error(loop["cast"]["out"][0], loop["truth"])
    print("mapper loop: pose errors", errors, "hit share", share, "mean |d - truth|", err)
    assert all(pose_error(MAPPER_HELD_OUT, p) > 10 * POSE_BOUND for p in poses)      # the raycast pose is none of the five views
    assert bool((loop["truth"] > FAR).all()) and bool((loop["truth"] < NEAR).all())
    for p in poses:
        t = render(p, H0, W0, PLANES, loop["Q"])
        assert bool((t > FAR).all()) and bool((t < NEAR).all()) and bool((t > MAPPER_MIN_DISP).all())
    assert all(e <= k * POSE_BOUND for k, e in enumerate(errors)), errors
    assert share >= HIT_SHARE, share
    # the loop's own numbers, as recorded: they come out of a Gauss-Newton loop, so another CPU or BLAS may move the last digits
    assert share == pytest.approx(0.8863, abs=0.01) and err == pytest.approx(3.687e-3, rel=0.05), (share, err)
    assert MEASURED_MAPPER_ERROR == pytest.approx(err, rel=0.05) and MEASURED_MAPPER_HIT_SHARE <= share + 0.01


# ---- integration: every decision --------------------------------------------------------------------------------------------------------
# A Q of powers of two and the identity pose: grid point (i, j, k) of a volume with voxel 1/64 and origin (-4/64, -2/64, 1) is the
# camera point ((i - 4) / 64, (j - 2) / 64, 1 + k / 64), and at k = 0 (z = 1) it projects exactly onto pixel (i, j).
def unit_setup(voxel=1.0 / 64, origin=(-4.0 / 64, -2.0 / 64, 1.0)):
    ops = ecm().ops
    Q = ops.q_matrix(64.0, 0.25, 4.0, 2.0)                                 # d = 16 / z
    return Q, ops.volume_matrices(Q, torch.eye(4, dtype=F64), origin, voxel)


def one_slice(disp, trunc=0.5, dims=(1, 4, 6), **kw):
    Q, m = unit_setup()
    return integrate_t(*empty(dims), disp, Q, m.G, m.C, trunc, **kw)


def test_projection_is_exact_on_the_unit_scene():
    Q, m = unit_setup()
    g = torch.tensor([3.0, 1.0, 0.0, 1.0], dtype=F64)
    h = m.G @ g
    assert (h[:3] / h[3]).tolist() == [3.0, 1.0, 16.0] and (m.C @ g).tolist() == [-1.0 / 64, -1.0 / 64, 1.0, 1.0]


def test_unusable_disparities_weights_and_masks_touch_nothing():
    d = torch.full((1, 4, 6), 8.0)                                         # z_meas = 2, z_vox = 1: s = 1, t = min(1, 2) = 1
    X, N, touched = one_slice(d)
    assert bool(touched.all()) and bool((X == 1).all()) and bool((N == 1).all())
    for bad in (NAN, INF, -INF, 0.0, -1.0):
        dd = d.clone()
        dd[0, 1, 2] = bad
        X, N, touched = one_slice(dd)
        assert int(touched.sum()) == 23 and not bool(touched[0, 1, 2]) and float(N[0, 1, 2]) == 0 and float(X[0, 1, 2]) == 1, bad
        w = torch.ones(1, 4, 6)
        w[0, 3, 5] = bad
        X, N, touched = one_slice(d, weight=w)
        assert int(touched.sum()) == 23 and not bool(touched[0, 3, 5]), bad
    v = torch.ones(1, 4, 6, dtype=torch.uint8)
    v[0, 0, 0] = 0
    assert int(one_slice(d, valid=v)[2].sum()) == 23
    assert int(one_slice(d, min_disp=8.0)[2].sum()) == 0 and int(one_slice(d, max_disp=8.0)[2].sum()) == 24
    assert int(one_slice(d, max_disp=7.5)[2].sum()) == 0


def test_truncation_boundaries():
    # z_vox = 1 exactly; z_meas = 16 / d.  s == -trunc is integrated with t = -1 and s == trunc with t = 1
    for d, trunc, want in ((32.0, 0.5, -1.0), (8.0, 1.0, 1.0), (8.0, 0.5, 1.0), (8.0, 2.0, 0.5), (32.0, 2.0, -0.25), (16.0, 0.5, 0.0)):
        X, N, touched = one_slice(torch.full((1, 4, 6), d), trunc=trunc)
        assert bool(touched.all()) and bool((X == want).all()) and bool((N == 1).all()), (d, trunc, X[0, 0, 0])
    X, N, touched = one_slice(torch.full((1, 4, 6), 64.0), trunc=0.5)                            # s = -0.75 < -trunc
    assert not bool(touched.any()) and bool((X == 1).all()) and bool((N == 0).all())
    below = float(torch.nextafter(f32(0.5), f32(0.0)))                                           # s = -0.5, trunc one fp32 ulp less
    assert not bool(one_slice(torch.full((1, 4, 6), 32.0), trunc=below)[2].any())


def test_pixel_rounding_boundary_and_the_image_border():
    # half a voxel of 1/64 off the origin puts u + 0.5 exactly on the boundary: u = i - 0.5 rounds up to pixel i
    Q, m = unit_setup(origin=(-4.5 / 64, -2.0 / 64, 1.0))
    d = torch.full((1, 4, 6), 8.0) + torch.arange(6) * 0.125               # the column can be read back from t
    X, N, touched = integrate_t(*empty((1, 4, 8)), d, Q, m.G, m.C, 64.0)
    h = m.G @ torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=F64)
    assert float(h[0] / h[3]) == 0.5                                       # grid i = 1 is u = 0.5: floor(1.0) = pixel 1
    z = 16.0 / d[0, 0].to(F64)
    want = ((z - 1.0) / 64.0).to(F32)
    # u = i - 0.5 rounds UP to pixel i: i = 0 (u = -0.5) reads pixel 0, i = 5 pixel 5, and i = 6, 7 leave the image
    assert touched[0, 0].tolist() == [True] * 6 + [False] * 2 and torch.equal(X[0, 0, :6], want)


def test_a_voxel_behind_the_camera_or_at_no_depth():
    Q, m = unit_setup(origin=(-4.0 / 64, -2.0 / 64, -2.0 / 64))           # k = 0, 1 behind, k = 2 at z = 0, k = 3 in front
    d = torch.full((1, 4, 6), 8.0)
    X, N, touched = integrate_t(*empty((4, 4, 6)), d, Q, m.G, m.C, 4.0)
    assert not bool(touched[:3].any()) and bool(touched[3].any())
    assert bool((X[:3] == 1).all()) and bool((N[:3] == 0).all())


def test_max_weight_clamps_the_sum_not_the_average():
    d = torch.full((1, 4, 6), 8.0)                                         # s = 1: t = 0.5 at trunc 2
    w = torch.full((1, 4, 6), 3.0)
    X, N, _ = one_slice(d, trunc=2.0, weight=w, max_weight=2.5)
    assert bool((N == 2.5).all()) and bool((X == 0.5).all())
    Q, m = unit_setup()
    d2 = torch.full((1, 4, 6), 32.0)                                       # s = -0.5: t = -0.5 at trunc 1
    X2, N2, _ = integrate_t(X, N, d2, Q, m.G, m.C, 1.0, weight=torch.full((1, 4, 6), 2.5), max_weight=2.5)
    assert bool((X2 == 0.0).all()) and bool((N2 == 2.5).all())             # (0.5 * 2.5 - 0.5 * 2.5) / 5


def test_two_views_in_one_call_are_two_calls():
    loop = closed_loop()
    ops = ecm().ops
    m = ops.volume_matrices(loop["Q"], torch.stack(VIEWS[:2]), ORIGIN, VOXEL)
    w = 0.5 + torch.rand(2, H0, W0, generator=torch.Generator().manual_seed(1))
    both = integrate_t(*empty(DIMS), loop["disp"][:2], loop["Q"], m.G, m.C, TRUNC, weight=w)
    first = integrate_t(*empty(DIMS), loop["disp"][:1], loop["Q"], m.G[0], m.C[0], TRUNC, weight=w[:1])
    second = integrate_t(first[0], first[1], loop["disp"][1:2], loop["Q"], m.G[1], m.C[1], TRUNC, weight=w[1:2])
    assert torch.equal(both[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(both[1], second[1])
    assert int((both[1] > 1.0).sum()) > 1000                               # many voxels were seen by both
    # the order is part of the definition: once max_weight clamps the first view's weight, the average depends on who came first
    clamped = integrate_t(*empty(DIMS), loop["disp"][:2], loop["Q"], m.G, m.C, TRUNC, weight=w, max_weight=0.75)
    swapped = integrate_t(*empty(DIMS), loop["disp"][:2].flip(0), loop["Q"], m.G.flip(0), m.C.flip(0), TRUNC, weight=w.flip(0), max_weight=0.75)
    assert not torch.equal(clamped[0], swapped[0])


# ---- raycast: every decision ------------------------------------------------------------------------------------------------------------
# A volume whose grid IS (x, y, d): R = Rinv = I, so pixel (x, y) marches along the grid's z axis from near_disp to far_disp
EYE = torch.eye(4, dtype=F64)


def slab(nz=8, ny=4, nx=6, surface=3.5):
    """tsdf = (surface - k) / 2 clamped to [-1, 1]: in front (k small) positive.  The ray runs from near to far, so it is cast
    from a small k to a large one by near_disp < ... -- the grid's k is the NEGATED disparity axis here: see cast()."""
    k = torch.arange(nz, dtype=F32).view(nz, 1, 1).expand(nz, ny, nx)
    return ((surface - k) / 2).clamp(-1, 1).contiguous(), torch.ones(nz, ny, nx)


FLIP = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, -1.0, 8.0], [0, 0, 0, 1.0]], dtype=F64)     # grid k = 8 - d; its own inverse


def cast(tsdf, wsum, near=8.0, far=1.0, step=0.5, size=None, **kw):
    nz, ny, nx = tsdf.shape
    return raycast_t(tsdf, wsum, FLIP, FLIP, size or (ny, nx), near, far, step, **kw)


def test_a_ray_finds_the_crossing_by_linear_interpolation():
    tsdf, wsum = slab()
    res = cast(tsdf, wsum)                                                 # k from 0 to 7 in 14 steps of 0.5
    assert float(res["n"][0, 0, 0]) == 14
    inner = res["out"][0, :3, :5]                                          # the last row and column have no cell: floor(p) = dim - 1
    assert bool((inner == 4.5).all()), inner                               # k = 3.5 is d = 4.5
    assert bool((res["out"][0, 3] == 0).all()) and bool((res["out"][0, :, 5] == 0).all())
    assert bool((res["hit_weight"][0, :3, :5] == 1).all()) and bool((res["hit_weight"][0, 3] == 0).all())
    for step in (0.25, 1.0, 0.7):
        assert bool((cast(tsdf, wsum, step=step)["out"][0, :3, :5] - 4.5).abs().max() < 1e-6), step


def test_a_ray_that_misses_the_box_and_one_that_starts_inside():
    tsdf, wsum = slab()
    res = cast(tsdf, wsum, size=(9, 11))                                   # pixels beyond the volume's 4 x 6 footprint
    assert bool((res["out"][0, 3:] == 0).all()) and bool((res["out"][0, :, 5:] == 0).all()) and bool((res["out"][0, :3, :5] == 4.5).all())
    res = cast(tsdf, wsum, near=40.0, far=20.0)                            # k from -32 to -12: in front of the box
    assert not bool(res["hit"].any()) and float(res["n"][0, 0, 0]) == 40
    res = cast(tsdf, wsum, near=6.0, far=2.0)                              # k from 2 to 6: starts and ends inside
    assert bool((res["out"][0, :3, :5] == 4.5).all())
    res = cast(tsdf, wsum, near=4.25, far=2.0)                             # starts behind the surface: no front face ahead
    assert not bool(res["hit"].any())


def test_a_back_face_ends_the_ray():
    tsdf, wsum = slab(nz=12)
    tsdf = tsdf.clone()
    tsdf[:2] = -0.5                                                        # behind something at k < 2, free from k = 2 on, a surface at 3.5
    res = cast(tsdf, wsum)
    assert not bool(res["hit"].any())                                      # (-0.5, +0.75) between k = 1 and 2 comes first
    assert float((cast(tsdf, wsum, near=5.75, far=1.0)["out"][0, :3, :5] - 4.5).abs().max()) < 1e-6   # from k = 2.25 on there is none


def test_an_invalid_sample_breaks_the_pair():
    tsdf, wsum = slab()
    wsum = wsum.clone()
    wsum[4, 1, 2] = 0                                                      # a corner of the cells k = 3 and k = 4 about (x, y) = (1..2, 0..1)
    res = cast(tsdf, wsum, step=1.0)                                       # samples at k = 0, 1, ..: the pair (3, 4) straddles 3.5
    out = res["out"][0]
    assert out[0, 1] == 0 and out[0, 2] == 0 and out[1, 1] == 0 and out[1, 2] == 0 and out[2, 3] == 4.5 and out[0, 0] == 4.5
    # with half steps the pair (3, 3.5): both samples lie in cell k = 3, whose upper corners include the unweighted voxel
    assert cast(tsdf, wsum)["out"][0, 1, 1] == 0
    wsum[4, 1, 2] = -1.0
    assert cast(tsdf, wsum, step=1.0)["out"][0, 1, 1] == 0                 # > 0, not != 0


def test_max_steps_and_the_last_cell():
    tsdf, wsum = slab()
    assert bool(cast(tsdf, wsum, max_steps=14)["hit"].any()) and not bool(cast(tsdf, wsum, max_steps=13)["hit"].any())
    tsdf, wsum = slab(surface=6.25)                                        # the crossing lies in the last cell, k = dim - 2 = 6
    res = cast(tsdf, wsum)
    assert float((res["out"][0, :3, :5] - 1.75).abs().max()) < 1e-6        # between the samples at k = 6 and 6.5; k = 7 has no cell
    tsdf, wsum = slab(nz=2, surface=0.5)                                   # a volume of one cell
    assert float((cast(tsdf, wsum, near=8.0, far=7.0625)["out"][0, :3, :5] - 7.5).abs().max()) < 1e-6   # k from 0 to 0.9375


# ---- volume_matrices --------------------------------------------------------------------------------------------------------------------
def test_volume_matrices_identities():
    ops = ecm().ops
    Q, Q_out = scene_q(H0, W0), ops.q_matrix(70.0, 0.3, 30.0, 21.0)
    T = torch.stack(VIEWS)
    m = ops.volume_matrices(Q, T, ORIGIN, VOXEL, Q_out)
    assert isinstance(m, ops.VolumeMatrices) and m._fields == ("G", "C", "R", "Rinv") and all(t.shape == (4, 4, 4) and t.dtype == F64 for t in m)
    S = torch.eye(4, dtype=F64)
    S[:3, :3] *= VOXEL
    S[:3, 3] = torch.tensor(ORIGIN, dtype=F64)
    eye = torch.eye(4, dtype=F64)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))    # noqa: E731
    assert close(m.C @ torch.linalg.inv(S), T) and close(Q @ m.G, m.C) and close(m.G @ torch.linalg.inv(S) @ torch.linalg.inv(T) @ Q, eye.expand(4, 4, 4))
    assert close(m.R @ m.Rinv, eye.expand(4, 4, 4)) and close(S @ m.R, torch.linalg.inv(T) @ Q_out) and close(Q_out @ m.Rinv, m.C)
    one = ops.volume_matrices(Q, T[1], ORIGIN, VOXEL, Q_out)
    assert all(t.shape == (4, 4) for t in one) and all(torch.equal(a, b[1]) for a, b in zip(one, m))
    same = ops.volume_matrices(Q, T, ORIGIN, VOXEL)
    assert torch.equal(same.Rinv, same.G)                                  # Q_out None is Q
    # grid point (i, j, k) is origin + voxel (i, j, k) in the world, and the first view's camera is the world
    g = m.C[0] @ torch.tensor([3.0, 5.0, 7.0, 1.0], dtype=F64)
    assert close(g[:3], torch.tensor(ORIGIN, dtype=F64) + VOXEL * torch.tensor([3.0, 5.0, 7.0], dtype=F64))


def test_volume_matrices_refusals():
    ops = ecm().ops
    Q, eye = scene_q(H0, W0), torch.eye(4, dtype=F64)
    for bad in (0.0, -1.0, NAN, INF, True, "v"):
        with pytest.raises(ValueError, match="voxel"):
            ops.volume_matrices(Q, eye, ORIGIN, bad)
    for bad in ((0.0, 1.0), (0.0, 1.0, NAN), (0.0, INF, 1.0), "abc", None, (0, 1, 2, 3), torch.zeros(2)):
        with pytest.raises(ValueError, match="origin"):
            ops.volume_matrices(Q, eye, bad, VOXEL)
    assert torch.equal(ops.volume_matrices(Q, eye, torch.tensor(ORIGIN, dtype=F64), VOXEL).C, ops.volume_matrices(Q, eye, list(ORIGIN), VOXEL).C)
    with pytest.raises(ValueError, match="Q is singular"):
        ops.volume_matrices(torch.zeros(4, 4, dtype=F64), eye, ORIGIN, VOXEL, Q)
    with pytest.raises(ValueError, match="Q_out is singular"):
        ops.volume_matrices(Q, eye, ORIGIN, VOXEL, torch.zeros(4, 4, dtype=F64))
    for bad in (Q.float(), torch.eye(3, dtype=F64), "Q", torch.full((4, 4), NAN, dtype=F64), torch.stack([Q, Q])):
        with pytest.raises(ValueError, match="volume_matrices: Q"):
            ops.volume_matrices(bad, eye, ORIGIN, VOXEL)
    for bad in (eye.float(), torch.eye(3, dtype=F64), None, torch.full((4, 4), INF, dtype=F64)):
        with pytest.raises(ValueError, match="volume_matrices: T"):
            ops.volume_matrices(Q, bad, ORIGIN, VOXEL)
    scaled, mirrored, skewed, bottom = eye.clone(), eye.clone(), eye.clone(), eye.clone()
    scaled[:3, :3] *= 1.001
    mirrored[0, 0] = -1.0
    skewed[0, 1] = 1e-3
    bottom[3, 0] = 1e-3
    for bad in (scaled, mirrored, skewed, bottom, torch.stack([eye, skewed])):
        with pytest.raises(ValueError, match="not rigid"):
            ops.volume_matrices(Q, bad, ORIGIN, VOXEL)
    nearly = eye.clone()
    nearly[0, 1] = 5e-7                                                    # inside stereo_rectify's 1e-6
    ops.volume_matrices(Q, nearly, ORIGIN, VOXEL)


# ---- the ops' refusals: all of this runs on CPU tensors ---------------------------------------------------------------------------------
def test_op_signatures():
    ops = ecm().ops
    sig = inspect.signature(ops.volume_integrate)
    assert list(sig.parameters) == ["tsdf", "wsum", "disp", "Q", "T", "origin", "voxel", "trunc", "valid", "weight", "max_weight",
                                    "min_disp", "max_disp"]
    assert [p.default for p in list(sig.parameters.values())[8:]] == [None, None, 64.0, 0.0, None]
    sig = inspect.signature(ops.volume_raycast)
    assert list(sig.parameters) == ["tsdf", "wsum", "Q_out", "T", "origin", "voxel", "size", "near_disp", "far_disp", "step", "max_steps",
                                    "with_weight"]
    assert [p.default for p in list(sig.parameters.values())[9:]] == [0.5, None, False]
    assert list(inspect.signature(ops.volume_matrices).parameters) == ["Q", "T", "origin", "voxel", "Q_out"]
    assert list(inspect.signature(ops.volume_new).parameters) == ["dims", "device"]


def test_volume_op_refusals():
    ops = ecm().ops
    Q, eye = scene_q(4, 8), torch.eye(4, dtype=F64)
    vol = lambda *d: (fake(*d), fake(*d))                                                        # noqa: E731
    z = fake(1, 4, 8)
    integ = lambda t=None, w=None, disp=z, T=eye, trunc=0.1, **kw: ops.volume_integrate(         # noqa: E731
        *(vol(3, 4, 5) if t is None else (t, w)), disp, Q, T, ORIGIN, VOXEL, trunc, **kw)
    cast = lambda t=None, w=None, T=eye, size=(4, 8), near=8.0, far=2.0, **kw: ops.volume_raycast(  # noqa: E731
        *(vol(3, 4, 5) if t is None else (t, w)), Q, T, ORIGIN, VOXEL, size, near, far, **kw)
    for kw, match in (({"trunc": 0.0}, "trunc"), ({"trunc": NAN}, "trunc"), ({"trunc": True}, "trunc"), ({"max_weight": 0.0}, "max_weight"),
                      ({"max_weight": INF}, "max_weight"), ({"min_disp": NAN}, "min_disp"), ({"min_disp": 2.0, "max_disp": 1.0}, "max_disp")):
        with pytest.raises(ValueError, match=match):
            integ(**kw)
    for kw, match in (({"near": 2.0}, "near_disp"), ({"far": 0.0}, "far_disp"), ({"far": -1.0}, "far_disp"), ({"near": INF}, "near_disp"),
                      ({"step": 0.0}, "step"), ({"step": NAN}, "step"), ({"max_steps": 0}, "max_steps"), ({"max_steps": 1.5}, "max_steps"),
                      ({"max_steps": MAX_STEPS + 1}, "max_steps"), ({"size": (4,)}, "size"), ({"size": (0, 8)}, "size")):
        with pytest.raises(ValueError, match=match):
            cast(**kw)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        integ(torch.ones(3, 4, 5), torch.zeros(3, 4, 5))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        cast(torch.ones(3, 4, 5), torch.zeros(3, 4, 5))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.volume_new((2, 2, 2), "cpu")
    for bad in ((2, 2), (0, 2, 2), (2, 2, 2.0), "dims", (True, 2, 2)):
        with pytest.raises(ValueError, match="dims"):
            ops.volume_new(bad, "cuda")
    # a tensor that requires grad is refused: forward only
    g = torch.zeros(3, 4, 5, requires_grad=True)
    for call in (lambda: integ(g, fake(3, 4, 5)), lambda: integ(fake(3, 4, 5), g), lambda: cast(g, fake(3, 4, 5)),
                 lambda: integ(disp=torch.zeros(1, 4, 8, requires_grad=True)), lambda: integ(weight=torch.zeros(1, 4, 8, requires_grad=True))):
        with pytest.raises(ValueError, match="requires grad"):
            call()
    for t, w in ((fake(3, 4, 5), fake(3, 4, 6)), (fake(4, 5), fake(4, 5)), (fake(3, 4, 5, dtype=F64), fake(3, 4, 5, dtype=F64))):
        with pytest.raises(RuntimeError):
            integ(t, w)
    with pytest.raises(RuntimeError, match="contiguous"):
        integ(fake(3, 5, 4).transpose(1, 2), fake(3, 4, 5))
    one = fake(3, 4, 5)
    with pytest.raises(RuntimeError, match="one tensor"):
        integ(one, one)
    with pytest.raises(RuntimeError, match="every dim >= 2"):
        cast(*vol(1, 4, 5))
    with pytest.raises(ValueError, match="one matrix, or one per view"):
        integ(disp=fake(2, 4, 8), T=torch.stack([eye] * 3))
    for kw, match in (({"valid": z}, "valid"), ({"weight": fake(1, 4, 9)}, "weight"), ({"weight": fake(1, 4, 8, dtype=F64)}, "weight")):
        with pytest.raises(RuntimeError, match=match):
            integ(**kw)
    # every operand on one device, in the colour ops' words: a foreign pointer never reaches a kernel
    elsewhere = lambda *shape: torch.zeros(*shape, device="meta").as_subclass(type(z))           # noqa: E731  (a tensor of another device)
    for call in (lambda: integ(disp=elsewhere(1, 4, 8)), lambda: integ(weight=elsewhere(1, 4, 8)),
                 lambda: integ(valid=elsewhere(1, 4, 8).to(torch.uint8)), lambda: integ(fake(3, 4, 5), elsewhere(3, 4, 5)),
                 lambda: cast(fake(3, 4, 5), elsewhere(3, 4, 5))):
        with pytest.raises(RuntimeError, match="is on .*: one device"):
            call()
    big = fake(4, 4, 5)
    with pytest.raises(RuntimeError, match="share memory"):                # one alias rule, by byte span, for every pair of planes
        integ(big[:3], big[1:])
    assert ops.check_volume_parameters(0.5) == (0.5, 64.0, 0.0, FLT_MAX)
    assert ops.check_raycast_parameters((4, 8), 8, 2) == ((4, 8), 8.0, 2.0, 0.5, MAX_STEPS)


# ---- the census of the sixth header -------------------------------------------------------------------------------------------------------
def header_prototypes():
    with open(os.path.join(INCLUDE, HEADER)) as f:
        return parse_header(f.read())


def test_the_registries():
    lib = ecm()._lib
    assert lib.REGISTRIES == (lib.TABLES, lib.EXTENSION_TABLES, lib.MOTION_TABLES) and len(lib.REGISTRIES) == 3
    assert tuple(lib.TABLES) == ("ecm_hip.h", "ecm_geometry.h", "ecm_rectify.h") and tuple(lib.EXTENSION_TABLES) == ("ecm_temporal.h",)
    assert tuple(lib.MOTION_TABLES) == ("ecm_motion.h",)
    rows = dict(lib._tables())
    assert len(rows) == sum(len(t) for reg in lib.REGISTRIES for t, _ in reg.values()) and not any(n in rows for n in ENTRIES)
    assert lib.LATER_REGISTRIES == (lib.VOLUME_TABLES,) and tuple(lib.VOLUME_TABLES) == (HEADER,)
    assert lib.VOLUME_TABLES[HEADER][0] is lib.VOLUME_PROTOTYPES and lib.VOLUME_TABLES[HEADER][1] == PREFIX
    every = dict(lib._all_tables())
    assert len(every) == len(rows) + len(ENTRIES) and all(n in every for n in ENTRIES) and all(every[n] == rows[n] for n in rows)


def test_header_table_and_package_literals_name_the_same_entries():
    lib = ecm()._lib
    parsed = header_prototypes()
    with open(os.path.join(INCLUDE, HEADER)) as f:
        by_text = set(re.findall(rf"\b({PREFIX}[a-z0-9_]+)\s*\(", _strip(f.read())))
    found = package_entry_names(PREFIX + "[a-z0-9_]+", "VOLUME_PROTOTYPES")
    assert sorted(parsed) == sorted(by_text) == sorted(lib.VOLUME_PROTOTYPES) == sorted(found) == sorted(ENTRIES)
    assert all(n.startswith(PREFIX) for n in parsed)
    assert all(a.startswith("ops.py:") for at in found.values() for a in at), found
    for registry in lib.REGISTRIES:
        for table, _ in registry.values():
            assert not set(table) & set(lib.VOLUME_PROTOTYPES)


def test_prototypes_match_the_header_type_by_type():
    table, parsed = ecm()._lib.VOLUME_PROTOTYPES, header_prototypes()
    assert compare(parsed, table) == []
    assert all(table[n] == parsed[n] for n in parsed)


def test_library_exports_every_row_and_load_types_it(lib_mod):
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(lib, n)] == [] and lib_mod.missing_symbols() == []
    table = lib_mod.VOLUME_PROTOTYPES
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
    assert ecm().ops.raycast_max_steps() == lib_mod.query("ecmv_raycast_max_steps") == MAX_STEPS


# ---- the refusal contract, with the devices hidden --------------------------------------------------------------------------------------
ROWS = [
    Row("ecmv_integrate_fwd",
        "tsdf:p wsum:p disp:p valid:o weight:o Q:p G:p C:p m_per_view=~0 nx=1 ny=1 nz=1 V=1 H=1 W=1 trunc=f0.1 max_weight=f64 "
        "min_disp=f0 max_disp=f100 stream:s", legal=[{"m_per_view": 1}, {"nx": 4}, {"nx": 2047, "ny": 1024, "nz": 1024}],
        # "nx * ny * nz >= 2^31, H * W >= 2^31, or 2^24 bricks or more" (a brick is 16 x 4 x 4 threads)
        unsup=[{"nx": 2048, "ny": 1024, "nz": 1024}, {"nx": 65536, "ny": 65536}, {"H": 65536, "W": 32768}, {"ny": 65536, "nz": 4096}],
        header=HEADER),
    Row("ecmv_raycast_fwd",
        "tsdf:p wsum:p R:p Rinv:p m_per_view=~0 out:p hit_weight:o nx=2 ny=2 nz=2 B=1 H=1 W=1 near_disp=f8 far_disp=f2 step=f0.5 "
        "max_steps=16 stream:s", inval=[{"nx": 1}, {"ny": 1}, {"nz": 1}],
        legal=[{"m_per_view": 1}, {"max_steps": "ecmv_raycast_max_steps+0"}],
        # "B * ceil(H / 16) * ceil(W / 16) >= 2^24, or max_steps > ecmv_raycast_max_steps()"
        unsup=[{"nx": 2048, "ny": 1024, "nz": 1024}, {"H": 65536, "W": 32768}, {"B": 65536, "H": 256, "W": 256},
               {"max_steps": "ecmv_raycast_max_steps+1"}], header=HEADER),
]
INT_CONSTS = ("ecmv_raycast_max_steps",)


@pytest.fixture(scope="module")
def results(lib_mod):
    """{call id: return value} of the rows above from one fresh child that sees no device (tests/abi_refusal_child.py)."""
    parsed = header_prototypes()
    calls = [{"id": f"const|{n}", "fn": n, "res": "i", "args": []} for n in INT_CONSTS]
    for row in ROWS:
        calls += calls_of(row, lambda q: parsed[q][1])
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


def test_every_entry_of_the_sixth_header_has_a_row():
    parsed = header_prototypes()
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    assert sorted(ent) == sorted(r.name for r in ROWS) and qry == {}       # no kernel needs scratch: no size query
    for r in ROWS:
        assert r.types == ent[r.name], r.name
    assert sorted(set(parsed) - set(ent)) == sorted(INT_CONSTS)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    row = next(r for r in ROWS if r.name == name)
    bad = classify(row, results)
    assert not bad, "\n" + _report(bad)
    assert results[f"{name}|accepted"] > 0                                 # the pointers are never dereferenced: no device, no crash
    assert results["const|ecmv_raycast_max_steps"] == MAX_STEPS


def test_further_refusals_of_the_entries(lib_mod):
    """What the rows cannot express: floats, and an output that is an input or another output.  Every call returns before any HIP
    call."""
    lib = lib_mod.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(10)]                    # never dereferenced
    names = ("disp", "valid", "weight", "Q", "G", "C")
    base = [("tsdf", p[0]), ("wsum", p[1])] + [(n, p[i + 2]) for i, n in enumerate(names)] + [
        ("per", 0), ("nx", 4), ("ny", 4), ("nz", 4), ("V", 1), ("H", 2), ("W", 2), ("trunc", 0.1), ("max_weight", 64.0), ("lo", 0.0),
        ("hi", 100.0), ("stream", None)]
    call = lambda **kw: lib.ecmv_integrate_fwd(*[kw.get(k, v) for k, v in base])                 # noqa: E731
    for out in ("tsdf", "wsum"):
        for i, n in enumerate(names):
            assert call(**{out: p[i + 2]}) == EINVAL, (out, n)
    assert call(wsum=p[0]) == EINVAL
    for name in ("trunc", "max_weight"):
        for bad in (0.0, -1.0, NAN, INF):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    for kw in ({"lo": NAN}, {"lo": INF}, {"hi": NAN}, {"lo": 2.0, "hi": 1.0}):
        assert call(**kw) == EINVAL, kw
    assert call(nx=2048, ny=1024, nz=1024) == EUNSUP
    names = ("tsdf", "wsum", "R", "Rinv")
    base = [(n, p[i]) for i, n in enumerate(names)] + [
        ("per", 0), ("out", p[4]), ("hit_weight", p[5]), ("nx", 4), ("ny", 4), ("nz", 4), ("B", 1), ("H", 2), ("W", 2), ("near", 8.0),
        ("far", 2.0), ("step", 0.5), ("max_steps", 16), ("stream", None)]
    call = lambda **kw: lib.ecmv_raycast_fwd(*[kw.get(k, v) for k, v in base])                   # noqa: E731
    for out in ("out", "hit_weight"):
        for i, n in enumerate(names):
            assert call(**{out: p[i]}) == EINVAL, (out, n)
    assert call(hit_weight=p[4]) == EINVAL
    for kw in ({"step": 0.0}, {"step": -1.0}, {"step": NAN}, {"step": INF}, {"near": 2.0}, {"near": 1.0}, {"far": 0.0}, {"far": -1.0},
               {"far": NAN}, {"near": NAN}, {"near": INF}, {"max_steps": 0}):
        assert call(**kw) == EINVAL, kw
    assert call(max_steps=MAX_STEPS + 1) == EUNSUP
    # no legal call is made here: this process may see a device, and the pointers are not device memory


# ---- StereoMapper -----------------------------------------------------------------------------------------------------------------------
def test_mapper_refusals_come_before_any_model_call():
    e = ecm()
    models, ops = e.models, e.ops
    net, Q = e.get_model("cmfsm"), ops.q_matrix(700.0, 0.25, 64.0, 32.0)
    sig = inspect.signature(models.StereoMapper.__init__)
    assert list(sig.parameters) == ["self", "model", "Q", "origin", "voxel", "dims", "trunc", "head", "max_weight", "min_disp",
                                    "odometry_kwargs"]
    assert [p.default for p in list(sig.parameters.values())[7:10]] == [2, 64.0, 1.0]
    assert models.Mapped._fields == models.Odometry._fields + ("world", "integrated", "frames")
    good = dict(origin=(-1.0, -1.0, 0.5), voxel=0.05, dims=(32, 32, 32), trunc=0.2)
    for kw, match in (({"origin": (0, 1)}, "origin"), ({"voxel": 0.0}, "voxel"), ({"dims": (32, 32)}, "dims"), ({"dims": (32, 0, 32)}, "dims"),
                      ({"trunc": -1.0}, "trunc"), ({"max_weight": 0.0}, "max_weight"), ({"min_disp": NAN}, "min_disp"), ({"head": 3}, "head"),
                      ({"step": 0}, "step"), ({"gate": -1}, "gate")):
        with pytest.raises(ValueError, match=match):
            models.StereoMapper(net, Q, **{**good, **kw})
    with pytest.raises(ValueError, match="model"):
        models.StereoMapper(torch.nn.Identity(), Q, **good)
    with pytest.raises(ValueError):
        models.StereoMapper(net, torch.zeros(4, 4, dtype=F64), **good)
    with pytest.raises(TypeError):
        models.StereoMapper(net, Q, **good, no_such_parameter=1)
    mapper = models.StereoMapper(net, Q, **good, step=1, iterations=3)
    assert not isinstance(mapper, torch.nn.Module) and isinstance(mapper.odometry, models.StereoOdometry)
    assert mapper.odometry.estimator["step"] == 1 and mapper.odometry.estimator["iterations"] == 3
    assert mapper.volume is None and mapper.frames == 0 and torch.equal(mapper.world, torch.eye(4, dtype=F64))
    for bad in (torch.zeros(2, 3, 64, 128), torch.zeros(3, 64, 128), None):
        with pytest.raises(ValueError, match="one pair at a time"):
            mapper(bad, bad)
    with pytest.raises(ValueError, match="no frame"):
        mapper.render()
    x = torch.zeros(1, 3, 64, 128)                                         # CPU tensors: a forward on them raises RuntimeError
    with pytest.raises(RuntimeError):
        mapper(x, x)
    with pytest.raises(ValueError, match="warp_matrix: T"):
        mapper(x, x, motion=torch.eye(4))
    mapper.reset()


def test_mapper_pose_bookkeeping_with_a_stub(monkeypatch):
    e = ecm()
    models, ops = e.models, e.ops
    Q = ops.q_matrix(700.0, 0.25, 64.0, 32.0)
    mapper = models.StereoMapper(e.get_model("cmfsm"), Q, (-1.0, -1.0, 0.5), 0.05, (8, 8, 8), 0.2)
    d = torch.full((1, 1, 4, 8), 5.0).as_subclass(OnDevice)
    std = torch.full((1, 1, 4, 8), 0.5).as_subclass(OnDevice)
    eye = torch.eye(4, dtype=F64)
    steps = [rigid(0.01, 0.0, 0.0, 0.1, 0.0, 0.0), rigid(0.0, 0.02, 0.0, 0.0, 0.0, 0.2), rigid(0.0, 0.0, 0.03, 0.0, 0.3, 0.0)]
    # frame 0 starts over; 1 converges; 2 does not (restarted); 3 converges
    script = [(eye, True), (steps[0], False), (eye, True), (steps[2], False)]
    seen = []

    def odometry(left, right):
        motion, restarted = script[len(seen)]
        seen.append(motion)
        return models.Odometry(d, std, d, d, std, d, motion[None].clone(), motion[None].clone(), None, restarted)

    integrated = []
    monkeypatch.setattr(mapper, "odometry", odometry)
    mapper.Q = Q
    odometry.reset = lambda: None
    monkeypatch.setattr(ops, "volume_new", lambda dims, device: (torch.ones(dims), torch.zeros(dims)))
    monkeypatch.setattr(ops, "volume_integrate", lambda tsdf, wsum, disp, Q_, T, *a, **kw: integrated.append((T.clone(), kw)))
    x = torch.zeros(1, 3, 4, 8)
    want_world = [eye, steps[0], steps[0], steps[2] @ steps[0]]
    want_frames, want_integrated = [1, 2, 2, 3], [True, True, False, True]
    for k in range(4):
        m = mapper(x, x)
        assert isinstance(m, models.Mapped)
        assert m.disparity is d and m.std is std and torch.equal(m.motion[0], script[k][0]) and m.restarted == script[k][1]
        assert torch.equal(m.world, want_world[k]) and m.integrated == want_integrated[k] and m.frames == want_frames[k], k
        assert m.world is not mapper.world
    assert len(integrated) == 3 and [torch.equal(t, w) for (t, _), w in zip(integrated, [want_world[0], want_world[1], want_world[3]])] == [True] * 3
    kw = integrated[0][1]
    assert sorted(kw) == ["max_weight", "min_disp", "valid", "weight"] and kw["max_weight"] == 64.0 and kw["min_disp"] == 1.0
    assert torch.equal(kw["valid"], d > 0) and torch.equal(kw["weight"], torch.full((1, 1, 4, 8), 4.0))
    mapper.volume[1].fill_(3.0)
    mapper.reset()
    assert bool((mapper.volume[0] == 1).all()) and bool((mapper.volume[1] == 0).all())
    assert mapper.frames == 0 and torch.equal(mapper.world, eye)
