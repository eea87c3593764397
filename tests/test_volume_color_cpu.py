"""Colour in the TSDF volume without a GPU: integrate_color_t, raycast_color_t and sample_t, fp64 torch
restatements of include/ecm_color.h written from the header's text, held bit for bit to integrate_t and raycast_t of
tests/test_disp_volume_cpu.py where the header says "as ecm_volume.h"; every decision of the definitions on hand-made volumes;
the closed loop (four analytic views of the three-plane scene, coloured by an affine function of the world point, integrated,
a fifth raycast, the mesh coloured) on the restatements; color.write_ply; the eighth header's census and refusal contract; the
refusals of color.* and models.ColorStereoMapper.  tests/test_hip_volume_color.py compares the device with the restatements.

Every operation of the restatements is one torch operation in the header's order (separate elementwise calls: nothing is fused),
so every value is the header's bit for bit."""
import ctypes as C
import inspect
import json
import os
import re
import struct
import subprocess
import sys

import pytest
import torch

import abi_refusal_child as child
from test_abi_refusals import EINVAL, EUNSUP, HIDE, Row, _report, calls_of, classify
from test_abi_types import INCLUDE, _strip, compare, lib_mod, package_entry_names, parse_header  # noqa: F401  (lib_mod: a fixture)
from test_disp_volume_cpu import (DIMS, F32, F64, FAR, FIFTH, H0, HIT_SHARE, MAPPER_HELD_OUT, MAPPER_MIN_DISP, MAPPER_STD, MAX_STEPS, NEAR, ORIGIN, TRUNC,
                                  VIEWS, VOXEL, W0, _row, closed_loop, empty, f32, integrate_t, mapper_loop, mapper_poses, raycast_t, scene_views,
                                  unit_setup)
from test_disp_warp_cpu import bits
from test_motion_align_cpu import PLANES, fake, render, scene_q
from test_volume_mesh_cpu import mesh_t, read_ply

HEADER = "ecm_color.h"
PREFIX = "ecmc_"
ENTRIES = ("ecmc_integrate_fwd", "ecmc_max_attributes", "ecmc_raycast_fwd", "ecmc_sample_fwd")
NAN, INF = float("nan"), float("inf")
MAX_ATTRIBUTES = 4


def ecm():
    import ecm_amd
    return ecm_amd


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def integrate_color_t(tsdf, wsum, attr, asum, disp, attributes, Q, G, Cm, trunc, valid=None, weight=None, max_weight=64.0, min_disp=0.0,
                      max_disp=None):
    """include/ecm_color.h's integration on CPU tensors: (tsdf, wsum, attr, asum, touched, coloured), new tensors; touched: some
    view updated the voxel's tsdf, coloured: some view updated its attributes.  The geometry step is integrate_t itself; the
    attribute step is the hook it calls after each view's tsdf step."""
    tr, mw = float(f32(trunc)), f32(max_weight)
    Y, Na = attr.clone(), asum.clone()
    coloured = torch.zeros(tsdf.shape, dtype=torch.bool)

    def attribute_step(v, ok, pixel, w, s):
        nonlocal Y, Na, coloured
        c = attributes[v][:, pixel[0], pixel[1]]                            # [A,nz,ny,nx]
        paint = ok & (s <= tr) & torch.isfinite(c).all(0)
        An = Na + w
        Yn = (Y * Na + c * w) / An
        Y, Na = torch.where(paint, Yn, Y), torch.where(paint, torch.minimum(An, mw), Na)
        coloured |= paint

    X, N, touched = integrate_t(tsdf, wsum, disp, Q, G, Cm, trunc, valid, weight, max_weight, min_disp, max_disp, seen=attribute_step)
    assert Y.shape == attr.shape
    return X, N, Y, Na, touched, coloured


def _sample(attr, asum, cell, q):
    """The sampling rule at the cells `cell` = [x, y, z] (long tensors) and positions q = [qx, qy, qz] (fp64) within them: [A, ...]
    fp32."""
    A = attr.shape[0]
    x, y, z = cell
    one = torch.ones_like(q[0])
    fx, fy, fz = (one - q[0], q[0]), (one - q[1], q[1]), (one - q[2], q[2])
    num, den = [torch.zeros_like(q[0]) for _ in range(A)], torch.zeros_like(q[0])
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                b = (fz[dz] * fy[dy]) * fx[dx]
                on = asum[z + dz, y + dy, x + dx] > 0
                for a in range(A):
                    num[a] = torch.where(on, num[a] + b * attr[a][z + dz, y + dy, x + dx].to(F64), num[a])
                den = torch.where(on, den + b, den)
    none = den == 0
    return torch.stack([torch.where(none, torch.zeros_like(den), num[a] / den).to(F32) for a in range(A)])


def raycast_color_t(tsdf, wsum, attr, asum, R, Rinv, size, near_disp, far_disp, step=0.5, max_steps=MAX_STEPS):
    """include/ecm_color.h's raycast on CPU tensors: raycast_t's dict (the march is raycast_t itself) plus colors [B,A,H,W] fp32,
    blended by the hook it calls at the hits."""
    B = R.shape[0] if R.dim() == 3 else 1
    cols = [torch.zeros((attr.shape[0],) + tuple(size), dtype=F32) for _ in range(B)]

    def blend_attributes(b, hit, cell, q):
        zero = torch.zeros_like(q[0])
        cols[b] = torch.where(hit, _sample(attr, asum, cell, [torch.where(hit, q[a], zero) for a in range(3)]), cols[b])

    cast = raycast_t(tsdf, wsum, R, Rinv, size, near_disp, far_disp, step, max_steps, at_hit=blend_attributes)
    return {**cast, "colors": torch.stack(cols)}


def sample_t(attr, asum, Minv, points):
    """include/ecm_color.h's point sampling on CPU tensors: [N,A] fp32."""
    nz, ny, nx = asum.shape
    dims = (nx, ny, nz)
    A, N = attr.shape[0], points.shape[0]
    if N == 0:
        return torch.zeros(0, A, dtype=F32)
    x, y, z = (points[:, a].to(F64) for a in range(3))
    g = [_row(Minv[r], x, y, z) for r in range(3)]
    outside = torch.zeros(N, dtype=torch.bool)
    for a in range(3):
        outside = outside | ~torch.isfinite(g[a]) | (g[a] < -0.5) | (g[a] > dims[a] - 0.5)
    zero = torch.zeros_like(x)
    gc = [torch.where(outside, zero, g[a]).clamp(0, dims[a] - 1) for a in range(3)]
    c = [torch.floor(gc[a]).clamp(0, dims[a] - 2) for a in range(3)]
    val = _sample(attr, asum, [t.long() for t in c], [gc[a] - c[a] for a in range(3)])             # [A,N]
    return torch.where(outside, torch.zeros_like(val), val).t().contiguous()


def empty_attributes(dims, A=3):
    return torch.zeros((A,) + tuple(dims), dtype=F32), torch.zeros(dims, dtype=F32)


# ---- the coloured scene the GPU test shares ---------------------------------------------------------------------------------------------
# colour a = AFFINE[a] . (X, Y, Z, 1) of the WORLD point, in about [0, 1] over the scene: the truth at any pose is known
AFFINE = torch.tensor([[0.25, 0.05, 0.02, 0.40], [-0.06, 0.22, 0.03, 0.45], [0.04, -0.03, 0.20, -0.10]], dtype=F64)

# The mean absolute colour error of the closed loop below, for the restatement on the CPU (not the device): of the raycast at
# FIFTH over the pixels that hit, and of the mesh's vertex colours.  Neither is rounding: a voxel takes the colour of the nearest
# PIXEL's surface point, which lies up to half a pixel's footprint and, across the band, up to trunc along the ray from the
# voxel, so the error scales with the colour gradient (up to 0.26 per metre) times one voxel (0.06 m): 1.6e-2 at worst for one
# voxel seen once; the averages over four views and eight corners come out thirty times below that.  The bounds are twice the
# measured values, which test_closed_loop_of_the_restatement prints.
MEASURED_COLOR_ERROR = 5.1e-4                                              # 5.019e-4 as printed
MEASURED_VERTEX_COLOR_ERROR = 6.1e-4                                       # 6.006e-4 as printed
COLOR_BOUND = 2 * MEASURED_COLOR_ERROR
VERTEX_COLOR_BOUND = 2 * MEASURED_VERTEX_COLOR_ERROR


def world_points(pose, H, W, Q):
    """The world point [3,H,W] (fp64) that every pixel of the analytic view at `pose` sees."""
    d = render(pose, H, W, PLANES, Q)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    P = torch.einsum("rc,chw->rhw", Q, torch.stack([xs, ys, d, torch.ones_like(xs)]))
    cam = torch.cat([P[:3] / P[3], torch.ones(1, H, W, dtype=F64)])
    return torch.einsum("rc,chw->rhw", torch.linalg.inv(pose), cam)[:3]


def affine_colors(points, A=3):
    """AFFINE at world points [3,...]: [A,...] fp64."""
    return torch.einsum("ac,c...->a...", AFFINE[:A, :3], points) + AFFINE[:A, 3].reshape((A,) + (1,) * (points.dim() - 1))


def scene_colors(poses=VIEWS, H=H0, W=W0, A=3):
    """[V,A,H,W] fp32: the colour image of each analytic view, rounded once."""
    Q = scene_q(H, W)
    return torch.stack([affine_colors(world_points(p, H, W, Q), A) for p in poses]).to(F32)


_LOOP = {}


def color_loop():
    """The restatement's coloured closed loop, computed once."""
    if not _LOOP:
        e = ecm()
        ops = e.ops
        disp, Q = scene_views()
        colors = scene_colors()
        m = ops.volume_matrices(Q, torch.stack(VIEWS), ORIGIN, VOXEL)
        tsdf, wsum, attr, asum, touched, coloured = integrate_color_t(*empty(DIMS), *empty_attributes(DIMS), disp, colors, Q, m.G, m.C, TRUNC)
        r = ops.volume_matrices(Q, FIFTH, ORIGIN, VOXEL)
        cast = raycast_color_t(tsdf, wsum, attr, asum, r.R, r.Rinv, (H0, W0), NEAR, FAR)
        M = e.mesh.mesh_matrix(ORIGIN, VOXEL)
        surface = mesh_t(tsdf, wsum, M)
        vertex_colors = sample_t(attr, asum, torch.linalg.inv(M), surface.vertices)
        _LOOP.update(tsdf=tsdf, wsum=wsum, attr=attr, asum=asum, touched=touched, coloured=coloured, cast=cast, Q=Q, disp=disp, colors=colors,
                     truth=affine_colors(world_points(FIFTH, H0, W0, Q)), mesh=surface, vertex_colors=vertex_colors,
                     vertex_truth=affine_colors(surface.vertices.to(F64).t()).t())
    return _LOOP


def color_error(colors, truth, hit):
    """mean |colors - truth| over the pixels (or vertices) of `hit` and the channels."""
    return float((colors.to(F64) - truth).abs()[..., hit].mean()) if colors.dim() == 3 else float((colors.to(F64) - truth).abs()[hit].mean())


def test_restatements_add_to_the_volume_ops_and_change_nothing():
    loop, base = color_loop(), closed_loop()
    for name in ("tsdf", "wsum"):
        assert torch.equal(bits(loop[name]), bits(base[name])), name
    assert torch.equal(loop["touched"], base["touched"])
    for name in ("out", "hit_weight"):
        assert torch.equal(bits(loop["cast"][name]), bits(base["cast"][name])), name
    assert torch.equal(loop["cast"]["hit"], base["cast"]["hit"]) and torch.equal(loop["cast"]["n"], base["cast"]["n"])
    # a dirty case as well: a used volume, masks, weights, gates, three views with their own matrices
    from test_hip_disp_volume import POSES, box, used_volume, views
    ops = ecm().ops
    dims = (5, 6, 9)
    origin, voxel = box(dims)
    d, Q, (valid, w) = views(3, 37, 61, 3, True)
    m = ops.volume_matrices(Q, torch.stack(POSES), origin, voxel)
    t0, w0 = used_volume(dims, 4)
    colors = dirty_attributes(3, 3, 37, 61, 8)
    kw = dict(max_weight=2.5, min_disp=0.05, max_disp=1.25 * 61 * 0.25 / 2.7)
    got = integrate_color_t(t0, w0, *used_attributes(dims, 3, 5), d, colors, Q, m.G, m.C, TRUNC, valid, w, **kw)
    want = integrate_t(t0, w0, d, Q, m.G, m.C, TRUNC, valid, w, **kw)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1])) and torch.equal(got[4], want[2])
    assert bool(got[5].any()) and bool((got[4] & ~got[5]).any()) and not bool((got[5] & ~got[4]).any())


def dirty_attributes(V, A, H, W, seed):
    """Attribute images with NaN and Inf sprinkled in (about 1 % each of NaN, Inf, -Inf per plane)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(V, A, H, W, generator=g)
    if min(H, W) > 2:
        r = torch.rand(V, A, H, W, generator=g)
        for k, bad in enumerate((NAN, INF, -INF)):
            a[(r >= 0.01 * k) & (r < 0.01 * (k + 1))] = bad
    return a


def used_attributes(dims, A, seed):
    """Attribute planes that have seen views before: attr in [0, 1], asum in [0, 3] with a third of it empty."""
    g = torch.Generator().manual_seed(seed)
    attr = torch.rand((A,) + tuple(dims), generator=g)
    asum = 3 * torch.rand(dims, generator=g)
    fresh = torch.rand(dims, generator=g) < 0.33
    return torch.where(fresh, torch.zeros(()), attr), torch.where(fresh, torch.zeros(()), asum)


# ---- integration: every decision --------------------------------------------------------------------------------------------------------
def paint_slice(disp, colors, trunc=0.5, dims=(1, 4, 6), start=None, **kw):
    """One view of the unit scene of tests/test_disp_volume_cpu.py (grid point (i, j, 0) is pixel (i, j) at z = 1; d = 16 / z)."""
    Q, m = unit_setup()
    A = colors.shape[1]
    vol = start or (empty(dims) + empty_attributes(dims, A))
    return integrate_color_t(*vol, disp, colors, Q, m.G, m.C, trunc, **kw)


def ramp(A=3, H=4, W=6):
    return (torch.arange(A * H * W, dtype=F32).reshape(1, A, H, W) + 1) / 128


def test_the_colour_band_ends_at_trunc_on_the_near_side():
    c = ramp()
    d = torch.full((1, 4, 6), 8.0)                                         # z_meas = 2, z_vox = 1: s = 1
    X, N, Y, Na, touched, coloured = paint_slice(d, c, trunc=1.0)          # s == trunc: coloured
    assert bool(coloured.all()) and torch.equal(Y, c[0][:, None]) and bool((Na == 1).all()) and bool((X == 1).all())
    just = torch.nextafter(f32(8.0), f32(0.0)).expand(1, 4, 6)             # z_meas one step above 2: s just above trunc
    X, N, Y, Na, touched, coloured = paint_slice(just, c, trunc=1.0)
    assert bool(touched.all()) and bool((X == 1).all()) and bool((N == 1).all())                 # free space is still carved
    assert not bool(coloured.any()) and bool((bits(Y) == 0).all()) and bool((bits(Na) == 0).all())
    below = float(torch.nextafter(f32(1.0), f32(0.0)))                     # the same s, trunc one fp32 step less
    assert not bool(paint_slice(d, c, trunc=below)[5].any()) and bool(paint_slice(d, c, trunc=below)[4].all())
    # behind the surface the band ends where the tsdf's does: s == -trunc is coloured, s < -trunc touches nothing at all
    X, N, Y, Na, touched, coloured = paint_slice(torch.full((1, 4, 6), 32.0), c, trunc=0.5)     # s = -0.5
    assert bool(coloured.all()) and bool((X == -1).all()) and torch.equal(Y, c[0][:, None])
    start = empty((1, 4, 6)) + tuple(t + 0.125 for t in empty_attributes((1, 4, 6)))
    out = paint_slice(torch.full((1, 4, 6), 64.0), c, trunc=0.5, start=start)                    # s = -0.75
    assert not bool(out[4].any()) and not bool(out[5].any())
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out[:4], start))


def test_a_value_that_is_not_finite_in_one_channel_skips_all_channels():
    d = torch.full((1, 4, 6), 16.0)                                        # s = 0
    for bad in (NAN, INF, -INF):
        c = ramp()
        c[0, 1, 2, 3] = bad
        X, N, Y, Na, touched, coloured = paint_slice(d, c)
        assert bool(touched.all()) and bool((N == 1).all()) and bool((X == 0).all()), bad
        assert int(coloured.sum()) == 23 and not bool(coloured[0, 2, 3]) and bool((bits(Y[:, 0, 2, 3]) == 0).all()) and float(Na[0, 2, 3]) == 0
        assert torch.equal(Y[:, 0][:, coloured[0]], c[0][:, coloured[0]])
    # an unusable disparity, weight or mask skips the colour with the tsdf
    dd = d.clone()
    dd[0, 0, 0] = NAN
    assert not bool(paint_slice(dd, ramp())[5][0, 0, 0]) and int(paint_slice(dd, ramp())[5].sum()) == 23
    w = torch.ones(1, 4, 6)
    w[0, 3, 5] = 0.0
    assert int(paint_slice(d, ramp(), weight=w)[5].sum()) == 23


def test_max_weight_clamps_asum_and_not_the_average():
    d = torch.full((1, 4, 6), 16.0)
    c = torch.full((1, 2, 4, 6), 0.5)
    X, N, Y, Na, _, _ = paint_slice(d, c, weight=torch.full((1, 4, 6), 3.0), max_weight=2.5)
    assert bool((Na == 2.5).all()) and bool((Y == 0.5).all()) and bool((N == 2.5).all())
    c2 = torch.full((1, 2, 4, 6), -0.5)
    out = paint_slice(d, c2, weight=torch.full((1, 4, 6), 2.5), max_weight=2.5, start=(X, N, Y, Na))
    assert bool((out[2] == 0.0).all()) and bool((out[3] == 2.5).all())     # (0.5 * 2.5 - 0.5 * 2.5) / 5
    # asum is the colour's own weight: a view that carves without colouring leaves it behind wsum
    out = paint_slice(torch.full((1, 4, 6), 4.0), c, trunc=0.5)            # s = 3 > trunc
    assert bool((out[1] == 1).all()) and bool((out[3] == 0).all())


def test_two_views_in_one_call_are_two_calls():
    loop = color_loop()
    ops = ecm().ops
    m = ops.volume_matrices(loop["Q"], torch.stack(VIEWS[:2]), ORIGIN, VOXEL)
    w = 0.5 + torch.rand(2, H0, W0, generator=torch.Generator().manual_seed(1))
    d, c, Q = loop["disp"], loop["colors"], loop["Q"]
    both = integrate_color_t(*empty(DIMS), *empty_attributes(DIMS), d[:2], c[:2], Q, m.G, m.C, TRUNC, weight=w)
    first = integrate_color_t(*empty(DIMS), *empty_attributes(DIMS), d[:1], c[:1], Q, m.G[0], m.C[0], TRUNC, weight=w[:1])
    second = integrate_color_t(*first[:4], d[1:2], c[1:2], Q, m.G[1], m.C[1], TRUNC, weight=w[1:2])
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(both[:4], second[:4]))
    assert int((both[3] > 1.0).sum()) > 1000                               # many voxels were coloured by both


# ---- the sampling rule ------------------------------------------------------------------------------------------------------------------
EYE = torch.eye(4, dtype=F64)


def test_an_uncoloured_corner_does_not_darken_the_blend():
    g = torch.Generator().manual_seed(2)
    attr = torch.rand(2, 2, 2, 2, generator=g)
    asum = torch.ones(2, 2, 2)
    asum[1, 0, 1] = 0.0                                                    # corner (dz, dy, dx) = (1, 0, 1)
    attr[:, 1, 0, 1] = 100.0                                               # what it holds must not be read into the result
    q = (0.25, 0.5, 0.75)                                                  # x, y, z
    got = sample_t(attr, asum, EYE, torch.tensor([q], dtype=F32))
    f = lambda t, d: t if d else 1.0 - t                                                         # noqa: E731
    num, den = [0.0, 0.0], 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                if (dz, dy, dx) != (1, 0, 1):
                    b = (f(q[2], dz) * f(q[1], dy)) * f(q[0], dx)
                    num = [num[a] + b * float(attr[a, dz, dy, dx]) for a in range(2)]
                    den += b
    assert den == 1.0 - (0.75 * 0.5) * 0.25 and got.tolist() == [[float(f32(num[a] / den)) for a in range(2)]]
    assert bool((got < 1.0).all())
    # a constant colour comes back whatever is missing
    flat = torch.full((1, 2, 2, 2), 0.7)
    assert sample_t(flat, asum, EYE, torch.tensor([q], dtype=F32)).item() == pytest.approx(0.7, abs=1e-7)
    # no coloured corner, and coloured corners whose weights are all zero: +0.0
    none = sample_t(attr, torch.zeros(2, 2, 2), EYE, torch.tensor([q], dtype=F32))
    assert bool((bits(none) == 0).all())
    lone = torch.zeros(2, 2, 2)
    lone[1, 1, 1] = 1.0
    assert bool((bits(sample_t(attr, lone, EYE, torch.tensor([[0.0, 0.5, 0.5]], dtype=F32))) == 0).all())    # b = 0 at the one corner
    assert bool((bits(sample_t(attr, -asum, EYE, torch.tensor([q], dtype=F32))) == 0).all())     # > 0, not != 0


def test_sampling_margin_clamp_and_nodes():
    g = torch.Generator().manual_seed(3)
    attr, asum = torch.rand(3, 3, 4, 5, generator=g), torch.ones(3, 4, 5)
    eps = 2.0 ** -20
    node = lambda x, y, z: attr[:, z, y, x].tolist()                                             # noqa: E731
    run = lambda *p: sample_t(attr, asum, EYE, torch.tensor([p], dtype=F32))[0].tolist()         # noqa: E731
    for x, y, z in ((0, 0, 0), (4, 3, 2), (2, 1, 1), (4, 0, 2), (0, 3, 0)):
        assert run(float(x), float(y), float(z)) == node(x, y, z)          # a node is its own value, bit for bit
    assert run(-0.5, 1.0, 2.0) == node(0, 1, 2) and run(-0.5 - eps, 1.0, 2.0) == [0.0] * 3
    assert run(4.5, 1.0, 2.0) == node(4, 1, 2) and run(4.5 + eps, 1.0, 2.0) == [0.0] * 3
    assert run(1.0, -0.5, 0.0) == node(1, 0, 0) and run(1.0, -0.5 - eps, 0.0) == [0.0] * 3
    assert run(1.0, 3.5, 0.0) == node(1, 3, 0) and run(1.0, 3.5 + eps, 0.0) == [0.0] * 3
    assert run(1.0, 2.0, -0.5) == node(1, 2, 0) and run(1.0, 2.0, -0.5 - eps) == [0.0] * 3
    assert run(1.0, 2.0, 2.5) == node(1, 2, 2) and run(1.0, 2.0, 2.5 + eps) == [0.0] * 3
    for bad in (NAN, INF, -INF):
        assert bool((bits(sample_t(attr, asum, EYE, torch.tensor([[1.0, bad, 1.0]], dtype=F32))) == 0).all())
    assert sample_t(attr, asum, EYE, torch.zeros(0, 3)).shape == (0, 3)
    # between nodes it is the trilinear blend, and a matrix moves the points
    mid = run(1.5, 2.5, 0.5)
    want = attr[:, 0:2, 2:4, 1:3].to(F64).mean((1, 2, 3))
    assert torch.allclose(torch.tensor(mid, dtype=F64), want, atol=1e-7)
    Minv = torch.linalg.inv(ecm().mesh.mesh_matrix((1.0, -2.0, 0.5), 0.25))
    assert sample_t(attr, asum, Minv, torch.tensor([[1.0 + 0.25 * 3, -2.0 + 0.25 * 2, 0.5 + 0.25]], dtype=F32))[0].tolist() == node(3, 2, 1)


def test_raycast_colours_on_the_slab():
    from test_disp_volume_cpu import FLIP, slab
    tsdf, wsum = slab()
    k = torch.arange(8, dtype=F32).view(8, 1, 1).expand(8, 4, 6)
    attr = torch.stack([k / 8, torch.full((8, 4, 6), 0.25)]).contiguous()
    res = raycast_color_t(tsdf, wsum, attr, torch.ones(8, 4, 6), FLIP, FLIP, (4, 6), 8.0, 1.0)
    assert bool((res["out"][0, :3, :5] == 4.5).all())                      # the surface at k = 3.5
    assert bool((res["colors"][0, 0, :3, :5] == 3.5 / 8).all()) and bool((res["colors"][0, 1, :3, :5] == 0.25).all())
    assert bool((bits(res["colors"][0][:, ~res["hit"][0]]) == 0).all())    # a hole is +0.0 in every plane
    nothing = raycast_color_t(tsdf, wsum, attr, torch.zeros(8, 4, 6), FLIP, FLIP, (4, 6), 8.0, 1.0)
    assert torch.equal(nothing["out"], res["out"]) and bool((bits(nothing["colors"]) == 0).all())


# ---- the closed loop --------------------------------------------------------------------------------------------------------------------
def test_closed_loop_of_the_restatement():
    loop = color_loop()
    cast = loop["cast"]
    hit = cast["hit"][0]
    share = float(hit.to(F64).mean())
    err = color_error(cast["colors"][0], loop["truth"], hit)
    verr = float((loop["vertex_colors"].to(F64) - loop["vertex_truth"]).abs().mean())
    print("colour loop: hit share", share, "mean |c - truth| raycast", err, "vertices", verr, "of", len(loop["mesh"].vertices),
          "coloured voxels", int(loop["coloured"].sum()), "of", int(loop["touched"].sum()), "touched")
    assert float(loop["truth"].min()) > 0.0 and float(loop["truth"].max()) < 1.0
    assert share >= HIT_SHARE, share
    # the colour holes are the disparity holes: every hit has a coloured corner, every hole is +0.0
    assert bool((cast["colors"][0][:, hit] > 0).all()) and bool((bits(cast["colors"][0][:, ~hit]) == 0).all())
    assert err <= MEASURED_COLOR_ERROR and MEASURED_COLOR_ERROR <= 1.25 * err, err            # the recorded value is the measured one
    assert verr <= MEASURED_VERTEX_COLOR_ERROR and MEASURED_VERTEX_COLOR_ERROR <= 1.25 * verr, verr
    assert len(loop["mesh"].vertices) > 1000 and bool((loop["vertex_colors"] > 0).all())
    assert torch.equal(loop["asum"] > 0, loop["coloured"]) and not bool((loop["coloured"] & ~loop["touched"]).any())
    assert int(loop["coloured"].sum()) < int(loop["touched"].sum())        # free space is carved, not coloured


# ---- the mapper's coloured loop -----------------------------------------------------------------------------------------------------------
# tests/test_disp_volume_cpu.py::mapper_loop with colour: the five analytic views along the screw motion, each integrated at the
# pose that the loop ESTIMATED for it (the restated motion estimate, composed as StereoMapper composes it) with the mapper's valid,
# weight and min_disp and with the colour image of the frame's TRUE pose, raycast at MAPPER_HELD_OUT and meshed in the world frame.
# The truth is the affine colour of the true scene at MAPPER_HELD_OUT, and at the vertices' own positions.  Measured on the CPU with
# the restatements (the test below prints them): beside the nearest-pixel read of the loop above they carry the accumulated pose
# error of four estimates, which puts a frame's colours on the volume slightly off.  models.ColorStereoMapper on the device is held
# to twice them.
MEASURED_MAPPER_COLOR_ERROR = 8.0e-4                                       # 7.911e-4 as printed
MEASURED_MAPPER_VERTEX_COLOR_ERROR = 1.0e-3                                # 9.974e-4 as printed, over 4490 vertices
MAPPER_COLOR_BOUND = 2 * MEASURED_MAPPER_COLOR_ERROR
MAPPER_VERTEX_COLOR_BOUND = 2 * MEASURED_MAPPER_VERTEX_COLOR_ERROR
_MAPPER_LOOP = {}


def color_mapper_loop():
    """The reference loop with colour, computed once."""
    if not _MAPPER_LOOP:
        e = ecm()
        ops = e.ops
        ref = mapper_loop()
        maps, Q = ref["maps"], ref["Q"]
        images = scene_colors(mapper_poses())
        std = torch.full((1, H0, W0), MAPPER_STD, dtype=F32)
        vol = empty(DIMS) + empty_attributes(DIMS)
        for k, world in enumerate(ref["worlds"]):
            m = ops.volume_matrices(Q, world, ORIGIN, VOXEL)
            vol = integrate_color_t(*vol, maps[k:k + 1], images[k:k + 1], Q, m.G, m.C, TRUNC, maps[k:k + 1] > 0, 1.0 / (std * std),
                                    min_disp=MAPPER_MIN_DISP)[:4]
        r = ops.volume_matrices(Q, MAPPER_HELD_OUT, ORIGIN, VOXEL)
        cast = raycast_color_t(*vol, r.R, r.Rinv, (H0, W0), NEAR, FAR)
        M = e.mesh.mesh_matrix(ORIGIN, VOXEL)
        surface = mesh_t(vol[0], vol[1], M)
        _MAPPER_LOOP.update(vol=vol, cast=cast, truth=affine_colors(world_points(MAPPER_HELD_OUT, H0, W0, Q)), mesh=surface,
                            vertex_colors=sample_t(vol[2], vol[3], torch.linalg.inv(M), surface.vertices),
                            vertex_truth=affine_colors(surface.vertices.to(F64).t()).t(), images=images)
    return _MAPPER_LOOP


def test_mapper_loop_of_the_restatements_with_colour():
    loop, ref = color_mapper_loop(), mapper_loop()
    assert torch.equal(bits(loop["vol"][0]), bits(ref["tsdf"])) and torch.equal(bits(loop["vol"][1]), bits(ref["wsum"]))
    assert torch.equal(bits(loop["cast"]["out"]), bits(ref["cast"]["out"]))
    hit = loop["cast"]["hit"][0]
    err = color_error(loop["cast"]["colors"][0], loop["truth"], hit)
    verr = float((loop["vertex_colors"].to(F64) - loop["vertex_truth"]).abs().mean())
    print("mapper colour loop: hit share", float(hit.to(F64).mean()), "mean |c - truth| raycast", err, "vertices", verr, "of", len(loop["mesh"].vertices))
    assert float(hit.to(F64).mean()) >= HIT_SHARE
    assert bool((loop["cast"]["colors"][0][:, hit] > 0).all()) and bool((bits(loop["cast"]["colors"][0][:, ~hit]) == 0).all())
    # the loop's own numbers, as recorded: they come out of a Gauss-Newton loop, so another CPU or BLAS may move the last digits
    assert err <= MEASURED_MAPPER_COLOR_ERROR and MEASURED_MAPPER_COLOR_ERROR <= 1.25 * err, err
    assert verr <= MEASURED_MAPPER_VERTEX_COLOR_ERROR and MEASURED_MAPPER_VERTEX_COLOR_ERROR <= 1.25 * verr, verr


# ---- color.write_ply --------------------------------------------------------------------------------------------------------------------
def test_write_ply_round_trip(tmp_path):
    e = ecm()
    color, mesh = e.color, e.mesh
    loop = color_loop()
    s = loop["mesh"]
    m = mesh.Mesh(s.vertices[:500], s.faces[(s.faces < 500).all(1)][:300], s.normals[:500], None)
    c = loop["vertex_colors"][:500].clone()
    c[0] = torch.tensor([-0.5, 1.5, NAN])
    c[1] = torch.tensor([0.6 / 255, 1.4 / 255, 254.6 / 255])
    for channels in (3, 4):
        cc = c if channels == 3 else torch.cat([c, torch.full((500, 1), 0.25)], 1)
        path = str(tmp_path / f"c{channels}.ply")
        color.write_ply(path, m, cc)
        with open(path, "rb") as f:
            raw = f.read()
        end = raw.index(b"end_header\n") + len(b"end_header\n")
        head = raw[:end].decode("ascii").splitlines()
        want_props = ["x", "y", "z", "nx", "ny", "nz"]
        names = ["red", "green", "blue", "alpha"][:channels]
        assert [ln for ln in head if ln.startswith("property uchar")] == [f"property uchar {n}" for n in names]
        assert [ln.split()[-1] for ln in head if ln.startswith("property float")] == want_props
        row = 24 + channels
        body = raw[end:]
        vrows = [body[k * row:(k + 1) * row] for k in range(500)]
        got = torch.tensor([list(r[24:]) for r in vrows], dtype=torch.uint8)
        want = torch.floor(torch.nan_to_num(cc.to(F64), nan=0.0).clamp(0, 1) * 255 + 0.5).to(torch.uint8)
        assert torch.equal(got, want) and got[0, :3].tolist() == [0, 255, 0] and got[1, :3].tolist() == [1, 1, 255]
        # without the colour properties it is mesh.write_ply's file
        plain = str(tmp_path / "plain.ply")
        mesh.write_ply(plain, m)
        with open(plain, "rb") as f:
            praw = f.read()
        pend = praw.index(b"end_header\n") + len(b"end_header\n")
        assert [ln for ln in head if not ln.startswith("property uchar")] == praw[:pend].decode("ascii").splitlines()
        assert b"".join(r[:24] for r in vrows) + body[500 * row:] == praw[pend:]
        props, v, f, _ = read_ply(plain)
        assert len(body[500 * row:]) == 13 * len(f)
    bare = mesh.Mesh(s.vertices[:4], torch.zeros(0, 3, dtype=torch.int32), None, None)
    color.write_ply(str(tmp_path / "bare.ply"), bare, torch.zeros(4, 3))
    assert os.path.getsize(str(tmp_path / "bare.ply")) > 4 * 15
    for bad in (torch.zeros(4, 2), torch.zeros(3, 3), torch.zeros(4), "c", None, torch.zeros(4, 5)):
        with pytest.raises(ValueError, match="colors"):
            color.write_ply(str(tmp_path / "bad.ply"), bare, bad)
    with pytest.raises(ValueError, match="a Mesh"):
        color.write_ply(str(tmp_path / "bad.ply"), (s.vertices, s.faces), torch.zeros(4, 3))


# ---- signatures and refusals: all of this runs on CPU tensors ---------------------------------------------------------------------------
def test_signatures_and_exports():
    e = ecm()
    color, models = e.color, e.models
    par = lambda f: list(inspect.signature(f).parameters)                                        # noqa: E731
    dflt = lambda f, k: [p.default for p in list(inspect.signature(f).parameters.values())[k:]]  # noqa: E731
    assert par(color.volume_attributes_new) == ["dims", "channels", "device"]
    assert par(color.volume_integrate) == ["tsdf", "wsum", "attr", "asum", "disp", "attributes", "Q", "T", "origin", "voxel", "trunc", "valid",
                                           "weight", "max_weight", "min_disp", "max_disp"]
    assert dflt(color.volume_integrate, 11) == [None, None, 64.0, 0.0, None]
    assert par(color.volume_raycast) == ["tsdf", "wsum", "attr", "asum", "Q_out", "T", "origin", "voxel", "size", "near_disp", "far_disp", "step",
                                         "max_steps", "with_weight"]
    assert dflt(color.volume_raycast, 11) == [0.5, None, False]
    assert par(color.volume_sample) == ["attr", "asum", "points", "origin", "voxel", "T"] and dflt(color.volume_sample, 5) == [None]
    assert par(color.mesh_colors) == ["m", "attr", "asum", "origin", "voxel", "T"] and dflt(color.mesh_colors, 5) == [None]
    assert par(color.write_ply) == ["path", "m", "colors"]
    assert color.max_attributes() == MAX_ATTRIBUTES == e.ops.disparity_warp_max_attributes()
    import importlib
    pkg = importlib.import_module("explicit-context-mapping-for-stereo-matching_amd")
    assert pkg.__all__[-2:] == ["color", "mesh"] and pkg.color is color and e.color is color
    assert issubclass(models.ColorStereoMapper, models.StereoMapper)
    assert par(models.ColorStereoMapper.__init__) == ["self", "model", "Q", "origin", "voxel", "dims", "trunc", "head", "max_weight", "min_disp",
                                                      "channels", "odometry_kwargs"]
    assert dflt(models.ColorStereoMapper.__init__, 7)[:4] == [2, 64.0, 1.0, 3]
    assert par(models.ColorStereoMapper.__call__) == ["self", "left", "right", "motion", "colors"]
    assert par(models.ColorStereoMapper.render_colors) == par(models.StereoMapper.render)
    assert dflt(models.ColorStereoMapper.render_colors, 1) == dflt(models.StereoMapper.render, 1)
    sig = inspect.signature(models.ColorStereoMapper.colored_mesh)
    assert list(sig.parameters) == ["self", "min_weight", "kw"] and sig.parameters["min_weight"].default == 0.0
    assert par(models.StereoMapper.__call__) == ["self", "left", "right", "motion"]


def test_color_op_refusals():
    e = ecm()
    color = e.color
    Q, eye = scene_q(4, 8), torch.eye(4, dtype=F64)
    D = (3, 4, 5)
    z, att = fake(1, 4, 8), fake(1, 3, 4, 8)
    base = lambda: dict(tsdf=fake(*D), wsum=fake(*D), attr=fake(3, *D), asum=fake(*D))           # noqa: E731

    def integ(disp=z, attributes=att, T=eye, trunc=0.1, **kw):
        planes = {**base(), **{k: kw.pop(k) for k in ("tsdf", "wsum", "attr", "asum") if k in kw}}
        return color.volume_integrate(planes["tsdf"], planes["wsum"], planes["attr"], planes["asum"], disp, attributes, Q, T, ORIGIN, VOXEL,
                                      trunc, **kw)

    def cast(T=eye, size=(4, 8), near=8.0, far=2.0, **kw):
        planes = {**base(), **{k: kw.pop(k) for k in ("tsdf", "wsum", "attr", "asum") if k in kw}}
        return color.volume_raycast(planes["tsdf"], planes["wsum"], planes["attr"], planes["asum"], Q, T, ORIGIN, VOXEL, size, near, far, **kw)

    # parameters, in the words of check_volume_parameters and check_raycast_parameters
    for kw, match in (({"trunc": 0.0}, "trunc"), ({"trunc": NAN}, "trunc"), ({"max_weight": 0.0}, "max_weight"), ({"min_disp": NAN}, "min_disp"),
                      ({"min_disp": 2.0, "max_disp": 1.0}, "max_disp")):
        with pytest.raises(ValueError, match=match):
            integ(**kw)
    for kw, match in (({"near": 2.0}, "near_disp"), ({"far": 0.0}, "far_disp"), ({"step": 0.0}, "step"), ({"max_steps": 0}, "max_steps"),
                      ({"max_steps": MAX_STEPS + 1}, "max_steps"), ({"size": (4,)}, "size")):
        with pytest.raises(ValueError, match=match):
            cast(**kw)
    with pytest.raises(ValueError, match="not rigid"):
        integ(T=eye * 2.0)
    # the planes, in _volume_planes' words
    for call in (integ, cast):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            call(tsdf=torch.ones(*D))
        with pytest.raises(RuntimeError, match="CPU tensor"):
            call(attr=torch.zeros(3, *D))
        with pytest.raises(RuntimeError, match="CPU tensor"):
            call(asum=torch.zeros(*D))
        for name in ("tsdf", "wsum", "attr", "asum"):
            shape = (3,) + D if name == "attr" else D
            with pytest.raises(ValueError, match=f"{name} requires grad"):
                call(**{name: torch.zeros(shape, requires_grad=True)})
        with pytest.raises(ValueError, match="a tensor"):
            call(attr="attr")
        with pytest.raises(RuntimeError, match="one tensor"):
            one = fake(*D)
            call(tsdf=one, wsum=one)
        for attr, asum in ((fake(3, 3, 4, 6), fake(*D)), (fake(*D), fake(*D)), (fake(3, *D), fake(3, 4, 6)), (fake(3, *D), fake(1, *D))):
            with pytest.raises(RuntimeError, match="of the volume's shape"):
                call(attr=attr, asum=asum)
        for A in (0, 5):
            with pytest.raises(RuntimeError, match="A in 1..4"):
                call(attr=fake(A, *D))
        with pytest.raises(RuntimeError, match="fp32"):
            call(attr=fake(3, *D, dtype=F64))
        with pytest.raises(RuntimeError, match="contiguous"):
            call(attr=fake(3, 3, 5, 4).transpose(2, 3))
        # aliasing: asum inside attr, attr over wsum
        big = fake(4, *D)
        with pytest.raises(RuntimeError, match="share memory"):
            call(attr=big[:3], asum=big[2])
        with pytest.raises(RuntimeError, match="share memory"):
            call(attr=big[:3], wsum=big[1])
        with pytest.raises(RuntimeError, match="share memory"):
            call(asum=big[0], tsdf=big[0])
    with pytest.raises(RuntimeError, match="every dim >= 2"):
        cast(tsdf=fake(1, 4, 5), wsum=fake(1, 4, 5), attr=fake(3, 1, 4, 5), asum=fake(1, 4, 5))
    # the views
    with pytest.raises(ValueError, match="one matrix, or one per view"):
        integ(disp=fake(2, 4, 8), attributes=fake(2, 3, 4, 8), T=torch.stack([eye] * 3))
    for bad in (fake(1, 2, 4, 8), fake(2, 3, 4, 8), fake(1, 3, 4, 9), fake(3, 4, 8), fake(1, 4, 8)):
        with pytest.raises(RuntimeError, match="want \\[V,A,H,W\\]"):
            integ(attributes=bad)
    with pytest.raises(RuntimeError, match="fp32"):
        integ(attributes=fake(1, 3, 4, 8, dtype=F64))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        integ(attributes=torch.zeros(1, 3, 4, 8))
    with pytest.raises(ValueError, match="attributes requires grad"):
        integ(attributes=torch.zeros(1, 3, 4, 8, requires_grad=True))
    with pytest.raises(ValueError, match="a tensor"):
        integ(attributes=None)
    for kw, match in (({"valid": z}, "valid"), ({"weight": fake(1, 4, 9)}, "weight")):
        with pytest.raises(RuntimeError, match=match):
            integ(**kw)
    # volume_attributes_new
    for bad in ((2, 2), (0, 2, 2), "dims"):
        with pytest.raises(ValueError, match="dims"):
            color.volume_attributes_new(bad, 3, "cuda")
    for bad in (0, 5, 1.5, True, None):
        with pytest.raises(ValueError, match="channels"):
            color.volume_attributes_new((2, 2, 2), bad, "cuda")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        color.volume_attributes_new((2, 2, 2), 3, "cpu")
    # volume_sample and mesh_colors
    samp = lambda attr=None, asum=None, points=None, origin=ORIGIN, voxel=VOXEL, T=None: color.volume_sample(  # noqa: E731
        fake(3, *D) if attr is None else attr, fake(*D) if asum is None else asum, fake(7, 3) if points is None else points, origin, voxel, T)
    for bad in (fake(7, 2), fake(7), fake(7, 3, 1)):
        with pytest.raises(RuntimeError, match="want \\[N,3\\]"):
            samp(points=bad)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        samp(points=torch.zeros(7, 3))
    with pytest.raises(RuntimeError, match="fp32"):
        samp(points=fake(7, 3, dtype=F64))
    with pytest.raises(ValueError, match="points requires grad"):
        samp(points=torch.zeros(7, 3, requires_grad=True))
    with pytest.raises(ValueError, match="a tensor"):
        samp(points=[[0.0, 0.0, 0.0]])
    elsewhere = lambda *shape: torch.zeros(*shape, device="meta").as_subclass(type(z))           # noqa: E731  (a tensor of another device)
    with pytest.raises(RuntimeError, match="one device"):
        samp(points=elsewhere(7, 3))
    with pytest.raises(RuntimeError, match="one device"):
        integ(attributes=elsewhere(1, 3, 4, 8))
    with pytest.raises(RuntimeError, match="every dim >= 2"):
        samp(attr=fake(3, 1, 4, 5), asum=fake(1, 4, 5))
    with pytest.raises(RuntimeError, match="A in 1..4"):
        samp(attr=fake(5, *D))
    with pytest.raises(ValueError, match="voxel"):
        samp(voxel=0.0)
    with pytest.raises(ValueError, match="origin"):
        samp(origin=(0.0, 1.0))
    with pytest.raises(ValueError, match="one \\[4,4\\] matrix"):
        samp(T=torch.stack([eye] * 2))
    with pytest.raises(ValueError, match="a Mesh"):
        color.mesh_colors((fake(7, 3), None), fake(3, *D), fake(*D), ORIGIN, VOXEL)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        color.mesh_colors(e.mesh.Mesh(torch.zeros(7, 3), torch.zeros(0, 3, dtype=torch.int32), None, None), fake(3, *D), fake(*D), ORIGIN, VOXEL)


def test_color_mapper_refusals_come_before_any_model_call():
    e = ecm()
    models, ops = e.models, e.ops
    net, Q = e.get_model("cmfsm"), ops.q_matrix(700.0, 0.25, 64.0, 32.0)
    good = dict(origin=(-1.0, -1.0, 0.5), voxel=0.05, dims=(32, 32, 32), trunc=0.2)
    for bad in (0, 5, 2.5, True):
        with pytest.raises(ValueError, match="channels"):
            models.ColorStereoMapper(net, Q, **good, channels=bad)
    for kw, match in (({"voxel": 0.0}, "voxel"), ({"dims": (32, 32)}, "dims"), ({"trunc": -1.0}, "trunc"), ({"step": 0}, "step")):
        with pytest.raises(ValueError, match=match):
            models.ColorStereoMapper(net, Q, **{**good, **kw})
    mapper = models.ColorStereoMapper(net, Q, **good, step=1)
    assert mapper.channels == 3 and mapper.volume is None and mapper.attributes is None and mapper.odometry.estimator["step"] == 1
    x = torch.zeros(1, 3, 64, 128)
    for bad in (torch.zeros(2, 3, 64, 128), torch.zeros(3, 64, 128), None):
        with pytest.raises(ValueError):
            mapper(bad, bad)
    for bad in (torch.zeros(1, 4, 64, 128), torch.zeros(3, 64, 128), "c"):
        with pytest.raises(ValueError, match="colors"):
            mapper(x, x, colors=bad)
    for bad in (torch.zeros(1, 3, 64, 127), torch.zeros(1, 3, 32, 128)):   # another size than the frames': before anything moves
        with pytest.raises(ValueError, match="one size"):
            mapper(x, x, colors=bad)
    with pytest.raises(ValueError, match="one device"):
        mapper(x, x, colors=torch.zeros(1, 3, 64, 128, device="meta"))
    assert mapper.frames == 0 and mapper.volume is None and torch.equal(mapper.world, torch.eye(4, dtype=F64))
    two = models.ColorStereoMapper(net, Q, **good, channels=2)
    with pytest.raises(ValueError, match="pass colors"):
        two(x, x)
    for call in (mapper.render_colors, mapper.colored_mesh, mapper.render, mapper.mesh):
        with pytest.raises(ValueError, match="no frame"):
            call()
    with pytest.raises(RuntimeError):
        mapper(x, x)                                                       # CPU tensors: a forward on them raises
    mapper.reset()


# ---- the census of the eighth header ------------------------------------------------------------------------------------------------------
def header_prototypes():
    with open(os.path.join(INCLUDE, HEADER)) as f:
        return parse_header(f.read())


def test_the_registries():
    lib = ecm()._lib
    assert lib.REGISTRIES == (lib.TABLES, lib.EXTENSION_TABLES, lib.MOTION_TABLES) and lib.LATER_REGISTRIES == (lib.VOLUME_TABLES,)
    assert lib.NEWER_REGISTRIES == (lib.MESH_TABLES,) and tuple(lib.MESH_TABLES) == ("ecm_mesh.h",)
    before = dict(lib._every_table())
    assert len(before) == sum(len(t) for reg in lib.REGISTRIES + lib.LATER_REGISTRIES + lib.NEWER_REGISTRIES for t, _ in reg.values())
    assert not any(n in before for n in ENTRIES)
    assert lib.NEWEST_REGISTRIES == (lib.COLOR_TABLES,) and tuple(lib.COLOR_TABLES) == (HEADER,)
    assert lib.COLOR_TABLES[HEADER][0] is lib.COLOR_PROTOTYPES and lib.COLOR_TABLES[HEADER][1] == PREFIX
    every = dict(lib._each_table())
    assert len(every) == len(before) + len(ENTRIES) and all(n in every for n in ENTRIES) and all(every[n] == before[n] for n in before)


def test_header_table_and_package_literals_name_the_same_entries():
    lib = ecm()._lib
    parsed = header_prototypes()
    with open(os.path.join(INCLUDE, HEADER)) as f:
        by_text = set(re.findall(rf"\b({PREFIX}[a-z0-9_]+)\s*\(", _strip(f.read())))
    found = package_entry_names(PREFIX + "[a-z0-9_]+", "COLOR_PROTOTYPES")
    assert sorted(parsed) == sorted(by_text) == sorted(lib.COLOR_PROTOTYPES) == sorted(found) == sorted(ENTRIES)
    assert all(n.startswith(PREFIX) for n in parsed)
    assert all(a.startswith("color.py:") for at in found.values() for a in at), found
    for registry in lib.REGISTRIES + lib.LATER_REGISTRIES + lib.NEWER_REGISTRIES:
        for table, _ in registry.values():
            assert not set(table) & set(lib.COLOR_PROTOTYPES)


def test_prototypes_match_the_header_type_by_type():
    table, parsed = ecm()._lib.COLOR_PROTOTYPES, header_prototypes()
    assert compare(parsed, table) == []
    assert all(table[n] == parsed[n] for n in parsed)


def test_library_exports_every_row_and_load_types_it(lib_mod):
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(lib, n)] == [] and lib_mod.missing_symbols() == []
    table = lib_mod.COLOR_PROTOTYPES
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
    assert lib_mod.query("ecmc_max_attributes") == MAX_ATTRIBUTES == lib_mod.query("ecmt_disparity_warp_max_attributes")


# ---- the refusal contract, with the devices hidden --------------------------------------------------------------------------------------
TOO_MANY_VOXELS = {"nx": 2048, "ny": 1024, "nz": 1024}
ROWS = [
    Row("ecmc_integrate_fwd",
        "tsdf:p wsum:p attr:p asum:p disp:p valid:o weight:o attributes:p Q:p G:p C:p m_per_view=~0 nx=1 ny=1 nz=1 A=?1 V=1 H=1 W=1 "
        "trunc=f0.1 max_weight=f64 min_disp=f0 max_disp=f100 stream:s",
        legal=[{"m_per_view": 1}, {"nx": 4}, {"A": 2}, {"A": 3}, {"A": "ecmc_max_attributes+0"}, {"nx": 2047, "ny": 1024, "nz": 1024}],
        # "A outside 1..ecmc_max_attributes(); nx * ny * nz >= 2^31, H * W >= 2^31, or 2^24 bricks or more"
        unsup=[{"A": "ecmc_max_attributes+1"}, TOO_MANY_VOXELS, {"nx": 65536, "ny": 65536}, {"H": 65536, "W": 32768}, {"ny": 65536, "nz": 4096}],
        header=HEADER),
    Row("ecmc_raycast_fwd",
        "tsdf:p wsum:p attr:p asum:p R:p Rinv:p m_per_view=~0 out:p hit_weight:o colors:p nx=2 ny=2 nz=2 A=?1 B=1 H=1 W=1 near_disp=f8 "
        "far_disp=f2 step=f0.5 max_steps=16 stream:s", inval=[{"nx": 1}, {"ny": 1}, {"nz": 1}],
        legal=[{"m_per_view": 1}, {"A": "ecmc_max_attributes+0"}, {"max_steps": "ecmv_raycast_max_steps+0"}],
        # "B * ceil(H / 16) * ceil(W / 16) >= 2^24, or max_steps > ecmv_raycast_max_steps()"
        unsup=[{"A": "ecmc_max_attributes+1"}, TOO_MANY_VOXELS, {"H": 65536, "W": 32768}, {"B": 65536, "H": 256, "W": 256},
               {"max_steps": "ecmv_raycast_max_steps+1"}], header=HEADER),
    Row("ecmc_sample_fwd", "attr:p asum:p Minv:p points:p out:p N=L1 nx=2 ny=2 nz=2 A=?1 stream:s", inval=[{"nx": 1}, {"ny": 1}, {"nz": 1}],
        legal=[{"A": "ecmc_max_attributes+0"}, {"N": (1 << 31) - 1}, {"nx": 2047, "ny": 1024, "nz": 1024}],
        # "A outside 1..ecmc_max_attributes(); N >= 2^31; nx * ny * nz >= 2^31"
        unsup=[{"A": "ecmc_max_attributes+1"}, {"N": 1 << 31}, {"N": 1 << 40}, TOO_MANY_VOXELS, {"nx": 65536, "ny": 65536}], header=HEADER),
]
INT_CONSTS = ("ecmc_max_attributes", "ecmv_raycast_max_steps")


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


def test_every_entry_of_the_eighth_header_has_a_row():
    parsed = header_prototypes()
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    assert sorted(ent) == sorted(r.name for r in ROWS) and qry == {}       # no kernel needs scratch: no size query
    for r in ROWS:
        assert r.types == ent[r.name], r.name
    assert sorted(set(parsed) - set(ent)) == ["ecmc_max_attributes"]


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    row = next(r for r in ROWS if r.name == name)
    bad = classify(row, results)
    assert not bad, "\n" + _report(bad)
    assert results[f"{name}|accepted"] > 0                                 # the pointers are never dereferenced: no device, no crash
    assert results["const|ecmc_max_attributes"] == MAX_ATTRIBUTES and results["const|ecmv_raycast_max_steps"] == MAX_STEPS


def test_further_refusals_of_the_entries(lib_mod):
    """What the rows cannot express: floats, and an output that is an input or another output.  Every call returns before any HIP
    call."""
    lib = lib_mod.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(12)]                    # never dereferenced
    outs = ("tsdf", "wsum", "attr", "asum")
    ins = ("disp", "valid", "weight", "attributes", "Q", "G", "C")
    base = [(n, p[i]) for i, n in enumerate(outs + ins)] + [
        ("per", 0), ("nx", 4), ("ny", 4), ("nz", 4), ("A", 3), ("V", 1), ("H", 2), ("W", 2), ("trunc", 0.1), ("max_weight", 64.0), ("lo", 0.0),
        ("hi", 100.0), ("stream", None)]
    call = lambda **kw: lib.ecmc_integrate_fwd(*[kw.get(k, v) for k, v in base])                 # noqa: E731
    for i, out in enumerate(outs):
        for j in range(len(ins)):
            assert call(**{out: p[4 + j]}) == EINVAL, (out, ins[j])
        for j in range(i):
            assert call(**{out: p[j]}) == EINVAL, (out, outs[j])
    for name in ("trunc", "max_weight"):
        for bad in (0.0, -1.0, NAN, INF):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    for kw in ({"lo": NAN}, {"lo": INF}, {"hi": NAN}, {"lo": 2.0, "hi": 1.0}):
        assert call(**kw) == EINVAL, kw
    assert call(A=0) == EUNSUP and call(A=5) == EUNSUP and call(nx=2048, ny=1024, nz=1024) == EUNSUP
    ins = ("tsdf", "wsum", "attr", "asum", "R", "Rinv")
    base = [(n, p[i]) for i, n in enumerate(ins)] + [
        ("per", 0), ("out", p[6]), ("hit_weight", p[7]), ("colors", p[8]), ("nx", 4), ("ny", 4), ("nz", 4), ("A", 3), ("B", 1), ("H", 2),
        ("W", 2), ("near", 8.0), ("far", 2.0), ("step", 0.5), ("max_steps", 16), ("stream", None)]
    call = lambda **kw: lib.ecmc_raycast_fwd(*[kw.get(k, v) for k, v in base])                   # noqa: E731
    for out in ("out", "hit_weight", "colors"):
        for i, n in enumerate(ins):
            assert call(**{out: p[i]}) == EINVAL, (out, n)
    assert call(hit_weight=p[6]) == EINVAL and call(colors=p[6]) == EINVAL and call(colors=p[7]) == EINVAL
    for kw in ({"step": 0.0}, {"step": NAN}, {"step": INF}, {"near": 2.0}, {"far": 0.0}, {"far": NAN}, {"near": NAN}, {"near": INF},
               {"max_steps": 0}):
        assert call(**kw) == EINVAL, kw
    assert call(max_steps=MAX_STEPS + 1) == EUNSUP and call(A=0) == EUNSUP and call(A=5) == EUNSUP
    ins = ("attr", "asum", "Minv", "points")
    base = [(n, p[i]) for i, n in enumerate(ins)] + [("out", p[4]), ("N", C.c_longlong(7)), ("nx", 4), ("ny", 4), ("nz", 4), ("A", 3),
                                                      ("stream", None)]
    call = lambda **kw: lib.ecmc_sample_fwd(*[kw.get(k, v) for k, v in base])                    # noqa: E731
    for i, n in enumerate(ins):
        assert call(out=p[i]) == EINVAL, n
    assert call(N=C.c_longlong(0)) == EINVAL and call(N=C.c_longlong(1 << 31)) == EUNSUP and call(A=5) == EUNSUP
    # no legal call is made here: this process may see a device, and the pointers are not device memory
