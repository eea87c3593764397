"""Colour in the TSDF volume (include/ecm_color.h states every operation): up to four attribute planes are
integrated with the disparity maps, raycast back with them and sampled at the vertices of the volume's mesh, and a PLY writer
for a coloured mesh.

Forward only, and a module of its own beside ops.py and mesh.py: the ops here are held to ops.py's forward-only operand contract
by their own test files (tests/test_volume_color_cpu.py, tests/test_hip_volume_color.py) until the table of that contract takes
them in.  tsdf, wsum, the raycast disparity and the mesh are what ops.volume_integrate, ops.volume_raycast and mesh.volume_mesh
give, bit for bit.

What the colour ops share with the plain ones is stated once, outside this module: ops._integrate_operands, ops._raycast_operands,
ops._volume_planes, ops._one_device and mesh._write_ply.  The ops here add the attribute planes, `attributes` and `colors`."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, mesh, ops


def max_attributes():
    """The most attribute planes a volume carries (a query of the library: no GPU needed)."""
    return int(_lib.query("ecmc_max_attributes"))


def _channels(who, channels):
    return ops._integer(who, "channels", channels, 1, max_attributes())


def volume_attributes_new(dims, channels, device):
    """The empty attribute planes of a volume of dims = (nz, ny, nx) on `device`: (attr, asum), fp32 [channels,nz,ny,nx] and
    [nz,ny,nx], all zeros.  channels in 1..max_attributes()."""
    who = "volume_attributes_new"
    dims = ops._volume_dims(who, dims)
    channels = _channels(who, channels)
    if torch.device(device).type != "cuda":
        raise RuntimeError(ops._CPU_TENSOR)
    return ops.torch.zeros((channels,) + dims, dtype=torch.float32, device=device), ops.torch.zeros(dims, dtype=torch.float32, device=device)


@torch.no_grad()
def volume_integrate(tsdf, wsum, attr, asum, disp, attributes, Q, T, origin, voxel, trunc, valid=None, weight=None, max_weight=64.0,
                     min_disp=0.0, max_disp=None):
    """ops.volume_integrate of the V views disp into (tsdf, wsum), and of their attributes ([V,A,H,W] fp32: colour, as given) into
    (attr, asum) of volume_attributes_new, IN PLACE, in one launch; returns the four tensors.  tsdf and wsum come out as
    ops.volume_integrate leaves them, bit for bit.  Where a view updates a voxel and the voxel is no more than trunc in FRONT of
    the measured surface either (so within trunc of it: the colour band is trunc wide on both sides), and all A attributes of
    the pixel are finite, attr <- (attr asum + c w) / (asum + w) and asum <- min(asum + w, max_weight) with the pixel's weight w.
    The pixel is the nearest one, as for the disparity; there is no view-angle weighting.  One thread per voxel, no atomics:
    bit-reproducible; a voxel no view colours keeps its bits.  include/ecm_color.h states every operation.  A static-scene
    model; every default is untested for quality."""
    who = "color.volume_integrate"
    (d, v, w), (held, *mats), dims, views, gates = ops._integrate_operands(
        who, dict(tsdf=tsdf, wsum=wsum, attr=attr, asum=asum), disp, Q, T, origin, voxel, trunc, valid, weight, max_weight, min_disp, max_disp,
        most_attributes=max_attributes(), attributes=attributes)
    A = int(attr.shape[0])
    if not isinstance(attributes, torch.Tensor):
        raise ValueError(f"{who}: attributes {type(attributes).__name__}: a tensor")
    ops._chk(attributes)
    ops._need(tuple(attributes.shape) == (views[0], A) + views[1:],
              lambda: f"{who}: attributes {tuple(attributes.shape)} against disp {tuple(d.shape)} and attr {tuple(attr.shape)}: want [V,A,H,W]")
    a = ops._c(attributes.detach())
    ops._one_device(who, tsdf=tsdf, wsum=wsum, attr=attr, asum=asum, disp=d, valid=v, weight=w, attributes=a)
    _lib.call("ecmc_integrate_fwd", ops._p(tsdf), ops._p(wsum), ops._p(attr), ops._p(asum), ops._p(d), ops._p(v), ops._p(w), ops._p(a), *mats,
              *dims, A, *views, *gates, ops._stream())
    return tsdf, wsum, attr, asum


@torch.no_grad()
def volume_raycast(tsdf, wsum, attr, asum, Q_out, T, origin, voxel, size, near_disp, far_disp, step=0.5, max_steps=None,
                   with_weight=False):
    """ops.volume_raycast of the volume, and the attributes at every hit: (out [B,1,H,W], colors [B,A,H,W]) fp32, or (out, colors,
    hit_weight) with with_weight=True.  out and hit_weight are ops.volume_raycast's, bit for bit.  A colour is the trilinear
    blend of attr over the corners of the hit's cell that were ever coloured (asum > 0), normalised by their weights, so an
    uncoloured corner does not darken it; a hole, and a hit with no coloured corner, is +0.0 in every plane.  One launch, one
    thread per pixel: bit-reproducible.  include/ecm_color.h states every operation."""
    (held, *mats), (out, hit), dims, views, march = ops._raycast_operands(
        "color.volume_raycast", dict(tsdf=tsdf, wsum=wsum, attr=attr, asum=asum), Q_out, T, origin, voxel, size, near_disp, far_disp, step,
        max_steps, with_weight, most_attributes=max_attributes())
    A = int(attr.shape[0])
    colors = ops.torch.empty(views[0], A, *views[1:], device=tsdf.device, dtype=torch.float32)
    _lib.call("ecmc_raycast_fwd", ops._p(tsdf), ops._p(wsum), ops._p(attr), ops._p(asum), *mats, ops._p(out), ops._p(hit), ops._p(colors),
              *dims, A, *views, *march, ops._stream())
    return (out, colors, hit) if with_weight else (out, colors)


@torch.no_grad()
def volume_sample(attr, asum, points, origin, voxel, T=None):
    """The attributes of the volume (attr, asum; every dim >= 2) at `points` ([N,3] fp32 on the device): [N,A] fp32.  The points
    are in the world frame (T None) or in the frame of the camera with pose T (float64 CPU [4,4], world to camera, rigid), as
    mesh.volume_mesh gives its vertices; origin and voxel place the grid.  A point is mapped to the grid by the inverse, taken
    on the host in fp64, of mesh.mesh_matrix(origin, voxel, T); within half a voxel of the grid's box it is clamped into the box
    and gets volume_raycast's blend there, and further out, or not finite, +0.0.  One thread per point: bit-reproducible."""
    who = "color.volume_sample"
    Minv = torch.linalg.inv(mesh.mesh_matrix(origin, voxel, T)).contiguous()                      # inv returns column-major strides: row-major for the kernel
    nz, ny, nx = ops._volume_planes(who, least=2, most_attributes=max_attributes(), attr=attr, asum=asum)
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"{who}: points {type(points).__name__}: a tensor")
    ops._no_grad_operands(who, points=points)
    ops._chk(points)
    ops._need(points.dim() == 2 and points.shape[1] == 3, lambda: f"{who}: points {tuple(points.shape)}: want [N,3]")
    ops._one_device(who, attr=attr, asum=asum, points=points)
    N, A = int(points.shape[0]), int(attr.shape[0])
    ops._need(N < 2 ** 31, lambda: f"{who}: {N} points: at most 2^31 - 1")
    out = ops.torch.empty((N, A), dtype=torch.float32, device=attr.device)
    if N:
        p = ops._c(points.detach())
        Md = Minv.to(attr.device)
        _lib.call("ecmc_sample_fwd", ops._p(attr), ops._p(asum), ops._p(Md), ops._p(p), ops._p(out), C.c_longlong(N), nx, ny, nz, A,
                  ops._stream())
    return out


def mesh_colors(m, attr, asum, origin, voxel, T=None):
    """volume_sample at the vertices of the Mesh m of mesh.volume_mesh: [N,A] fp32.  T is the T the mesh was extracted with."""
    if not isinstance(m, mesh.Mesh):
        raise ValueError(f"color.mesh_colors: m {type(m).__name__}: a Mesh")
    return volume_sample(attr, asum, m.vertices, origin, voxel, T)


def write_ply(path, m, colors):
    """mesh.write_ply's file for the Mesh m with `property uchar red green blue` (colors [N,3]) or `red green blue alpha` ([N,4])
    behind the floats of every vertex, by the same writer (mesh._write_ply).  A colour c is stored as
    floor(clamp(c, 0, 1) * 255 + 0.5), computed in fp64 (a NaN as 0): the caller de-normalises its attributes into [0, 1] first."""
    if colors is None:
        raise ValueError("color.write_ply: colors None: [N,3] or [N,4]")   # None is the writer's "no colour": mesh.write_ply
    mesh._write_ply(path, m, colors, "color.write_ply")
