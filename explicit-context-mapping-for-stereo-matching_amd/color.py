"""Colour in the TSDF volume (include/ecm_color.h states every operation): up to four attribute planes are
integrated with the disparity maps, raycast back with them and sampled at the vertices of the volume's mesh, and a PLY writer
for a coloured mesh.

Forward only, and a module of its own beside ops.py and mesh.py: the ops here are held to ops.py's forward-only operand contract
by their own test files (tests/test_volume_color_cpu.py, tests/test_hip_volume_color.py) until the table of that contract takes
them in.  tsdf, wsum, the raycast disparity and the mesh are what ops.volume_integrate, ops.volume_raycast and mesh.volume_mesh
give, bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
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


def _attribute_planes(who, attr, asum, dims=None, least=1, others=()):
    """The attribute planes of a volume after their refusals, in the words of ops._volume_planes: fp32 on the device, attr
    [A,nz,ny,nx] with A in 1..max_attributes() and asum [nz,ny,nx] (of the volume's shape `dims`, where given), contiguous (they
    are used in place), not requiring grad, and sharing no memory with one another or with `others`.  Returns (A, nz, ny, nx)."""
    for name, t in (("attr", attr), ("asum", asum)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} {type(t).__name__}: a tensor")
        if t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad: the volume ops are forward only")
    ops._chk(attr, asum)
    ops._need(asum.dim() == 3 and attr.dim() == 4 and attr.shape[1:] == asum.shape and all(n >= least for n in asum.shape)
              and (dims is None or tuple(asum.shape) == tuple(dims)),
              lambda: f"{who}: attr {tuple(attr.shape)}, asum {tuple(asum.shape)}: [A,nz,ny,nx] and [nz,ny,nx]"
              + (f" of the volume's shape {tuple(dims)}" if dims is not None else f", every dim >= {least}"))
    ops._need(1 <= attr.shape[0] <= max_attributes(), lambda: f"{who}: attr {tuple(attr.shape)}: A in 1..{max_attributes()}")
    ops._need(attr.is_contiguous() and asum.is_contiguous(), lambda: f"{who}: attr and asum must be contiguous")
    spans = [(name, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for name, t in (("attr", attr), ("asum", asum)) + tuple(others)]
    for i, (a, lo, hi) in enumerate(spans):
        for b, lo2, hi2 in spans[i + 1:]:
            ops._need(hi <= lo2 or hi2 <= lo, lambda: f"{who}: {a} and {b} share memory")
    return (int(attr.shape[0]),) + tuple(int(n) for n in asum.shape)


def _one_device(who, **ts):
    """Every tensor given (None: not passed) lies on the device of the first: the library takes pointers of one device."""
    first = None
    for name, t in ts.items():
        if t is None:
            continue
        if first is None:
            first = (name, t.device)
        ops._need(t.device == first[1], lambda: f"{who}: {name} is on {t.device}, {first[0]} on {first[1]}: one device")


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
    trunc, max_weight, lo, hi = ops.check_volume_parameters(trunc, max_weight, min_disp, max_disp, who)
    m = ops.volume_matrices(Q, T, origin, voxel)
    ops._no_grad_operands(who, disp=disp, valid=valid, weight=weight, attributes=attributes)
    nz, ny, nx = ops._volume_planes(who, tsdf, wsum)
    A = _attribute_planes(who, attr, asum, (nz, ny, nx), others=(("tsdf", tsdf), ("wsum", wsum)))[0]
    d, v = ops._filter_planes(who, disp, valid)
    V, H, W = d.shape
    if m.G.dim() == 3 and m.G.shape[0] != V:
        raise ValueError(f"{who}: T {tuple(T.shape)} against disp {tuple(d.shape)}: one matrix, or one per view")
    w = None if weight is None else ops._c(ops._plane_like(who, "weight", weight, d, ((torch.float32,)), "fp32"))
    if not isinstance(attributes, torch.Tensor):
        raise ValueError(f"{who}: attributes {type(attributes).__name__}: a tensor")
    ops._chk(attributes)
    ops._need(tuple(attributes.shape) == (V, A, H, W),
              lambda: f"{who}: attributes {tuple(attributes.shape)} against disp {tuple(d.shape)} and attr {tuple(attr.shape)}: want [V,A,H,W]")
    a = ops._c(attributes.detach())
    _one_device(who, tsdf=tsdf, wsum=wsum, attr=attr, asum=asum, disp=d, valid=v, weight=w, attributes=a)
    n = m.G.numel()
    mats = torch.cat([Q.detach().reshape(-1), m.G.reshape(-1), m.C.reshape(-1)]).to(d.device)        # one host-to-device copy
    at = mats.data_ptr()
    _lib.call("ecmc_integrate_fwd", ops._p(tsdf), ops._p(wsum), ops._p(attr), ops._p(asum), ops._p(d), ops._p(v), ops._p(w), ops._p(a),
              C.c_void_p(at), C.c_void_p(at + 128), C.c_void_p(at + 128 + 8 * n), int(m.G.dim() == 3), nx, ny, nz, A, V, H, W, trunc,
              max_weight, lo, hi, ops._stream())
    return tsdf, wsum, attr, asum


@torch.no_grad()
def volume_raycast(tsdf, wsum, attr, asum, Q_out, T, origin, voxel, size, near_disp, far_disp, step=0.5, max_steps=None,
                   with_weight=False):
    """ops.volume_raycast of the volume, and the attributes at every hit: (out [B,1,H,W], colors [B,A,H,W]) fp32, or (out, colors,
    hit_weight) with with_weight=True.  out and hit_weight are ops.volume_raycast's, bit for bit.  A colour is the trilinear
    blend of attr over the corners of the hit's cell that were ever coloured (asum > 0), normalised by their weights, so an
    uncoloured corner does not darken it; a hole, and a hit with no coloured corner, is +0.0 in every plane.  One launch, one
    thread per pixel: bit-reproducible.  include/ecm_color.h states every operation."""
    who = "color.volume_raycast"
    (H, W), near_disp, far_disp, step, max_steps = ops.check_raycast_parameters(size, near_disp, far_disp, step, max_steps, who)
    m = ops.volume_matrices(Q_out, T, origin, voxel)
    nz, ny, nx = ops._volume_planes(who, tsdf, wsum, least=2)
    A = _attribute_planes(who, attr, asum, (nz, ny, nx), others=(("tsdf", tsdf), ("wsum", wsum)))[0]
    _one_device(who, tsdf=tsdf, wsum=wsum, attr=attr, asum=asum)
    B = m.R.shape[0] if m.R.dim() == 3 else 1
    n = m.R.numel()
    dev = tsdf.device
    mats = torch.cat([m.R.reshape(-1), m.Rinv.reshape(-1)]).to(dev)
    at = mats.data_ptr()
    out = ops.torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
    colors = ops.torch.empty(B, A, H, W, device=dev, dtype=torch.float32)
    hit = ops.torch.empty(B, 1, H, W, device=dev, dtype=torch.float32) if with_weight else None
    _lib.call("ecmc_raycast_fwd", ops._p(tsdf), ops._p(wsum), ops._p(attr), ops._p(asum), C.c_void_p(at), C.c_void_p(at + 8 * n),
              int(m.R.dim() == 3), ops._p(out), ops._p(hit), ops._p(colors), nx, ny, nz, A, B, H, W, near_disp, far_disp, step, max_steps,
              ops._stream())
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
    A, nz, ny, nx = _attribute_planes(who, attr, asum, least=2)
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"{who}: points {type(points).__name__}: a tensor")
    if points.requires_grad:
        raise ValueError(f"{who}: points requires grad: the volume ops are forward only")
    ops._chk(points)
    ops._need(points.dim() == 2 and points.shape[1] == 3, lambda: f"{who}: points {tuple(points.shape)}: want [N,3]")
    _one_device(who, attr=attr, asum=asum, points=points)
    N = int(points.shape[0])
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
    behind the floats of every vertex.  A colour c is stored as floor(clamp(c, 0, 1) * 255 + 0.5), computed in fp64 (a NaN as 0):
    the caller de-normalises its attributes into [0, 1] first."""
    if not isinstance(m, mesh.Mesh):
        raise ValueError(f"color.write_ply: mesh {type(m).__name__}: a Mesh")
    if not isinstance(colors, torch.Tensor) or colors.dim() != 2 or colors.shape[1] not in (3, 4) or colors.shape[0] != m.vertices.shape[0]:
        raise ValueError(f"color.write_ply: colors {tuple(getattr(colors, 'shape', ()))!r} against vertices {tuple(m.vertices.shape)}: [N,3] or [N,4]")
    v, f = m.vertices.detach().cpu().to(torch.float32), m.faces.detach().cpu().to(torch.int32)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"color.write_ply: vertices {tuple(v.shape)}, faces {tuple(f.shape)}: [N,3] and [F,3]")
    names = ["x", "y", "z"]
    if m.normals is not None:
        n = m.normals.detach().cpu().to(torch.float32)
        if n.shape != v.shape:
            raise ValueError(f"color.write_ply: normals {tuple(n.shape)} against vertices {tuple(v.shape)}")
        v, names = torch.cat([v, n], 1), names + ["nx", "ny", "nz"]
    c = torch.nan_to_num(colors.detach().cpu().to(torch.float64), nan=0.0)
    c = torch.floor(c.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
    channels = ["red", "green", "blue", "alpha"][:c.shape[1]]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + [f"property float {n}" for n in names] \
        + [f"property uchar {n}" for n in channels] + [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(v.shape[0], dtype=np.dtype([("f", "<f4", (v.shape[1],)), ("c", "u1", (c.shape[1],))]))       # packed: no padding
    rows["f"], rows["c"] = v.numpy(), c.numpy()
    tris = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    tris["n"], tris["i"] = 3, f.numpy()
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(rows.tobytes())
        out.write(tris.tobytes())
