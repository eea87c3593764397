"""The triangle mesh of a TSDF volume (include/ecm_mesh.h states every operation): marching tetrahedra on
the device, as an indexed mesh with shared vertices, per-vertex normals and a consistent winding, and a PLY writer for it.

Forward only, and a module of its own beside ops.py: the ops here are held to ops.py's forward-only operand contract by their
own test file (tests/test_hip_volume_mesh.py) until the table of that contract takes them in.  The one PLY writer is here
(_write_ply): write_ply and color.write_ply are calls of it, without and with vertex colours."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib, ops

# What volume_mesh returns: vertices [N,3] fp32, faces [F,3] int32 (vertex numbers, counter-clockwise seen from free space),
# normals [N,3] fp32 or None (unit length, towards free space) and weight [N] fp32 or None (the interpolated wsum).
Mesh = collections.namedtuple("Mesh", "vertices faces normals weight")

_EYE = torch.eye(4, dtype=torch.float64)


def mesh_tile():
    """The points of one tile of the mesh ops' stream compaction (a query of the library: no GPU needed)."""
    return int(_lib.query("ecms_mesh_tile"))


def mesh_brick():
    """The points (x, y, z) of one classification brick of the mesh ops (a query of the library: no GPU needed)."""
    return tuple(int(_lib.query("ecms_mesh_brick", axis)) for axis in range(3))


def mesh_matrix(origin, voxel, T=None):
    """The grid-to-output matrix M of volume_mesh, float64 [4,4] on the CPU: S = [[voxel I, origin], [0, 1]] for T None (the world
    frame) and T S for a rigid T (world to camera: that camera's frame), formed and refused as ops.volume_matrices forms its C."""
    if T is not None and not (isinstance(T, torch.Tensor) and T.dim() == 2):
        raise ValueError(f"volume_mesh: T {tuple(getattr(T, 'shape', ()))!r}: one [4,4] matrix, or None")
    return ops.volume_matrices(_EYE, _EYE if T is None else T, origin, voxel).C


@torch.no_grad()
def volume_mesh(tsdf, wsum, origin, voxel, T=None, min_weight=0.0, with_normals=True, with_weight=False):
    """The zero level of the volume (tsdf, wsum; fp32 [nz,ny,nx] on the device, every dim >= 2) as Mesh(vertices, faces, normals,
    weight).  Every grid cube whose eight corners have wsum > min_weight and a finite tsdf is split into six tetrahedra, the same
    way in every cube, and each tetrahedron gives the triangles of its sign pattern (tsdf > 0 is positive; +-0 is negative); a
    vertex lies on a grid edge, a face diagonal or a body diagonal where the sign changes, at the linear zero of tsdf, and is
    shared by every triangle about it, so away from the volume's boundary and its unweighted regions the surface is closed and
    consistently oriented.  Vertices are in the world frame (T None) or in the frame of the camera with pose T (float64 CPU [4,4],
    world to camera, rigid); origin and voxel place the grid as in volume_matrices.  Normals are the normalised finite
    differences of tsdf, interpolated along the edge; they and the winding point to free space.  Two library calls with one
    host synchronisation between them (the counts size the outputs exactly); an empty mesh skips the second.  No atomics:
    bit-reproducible, vertices in the order (grid point, direction), faces in the order (cube, tetrahedron, triangle).  About twice
    the triangles of marching cubes, some of them slivers, and zero-area triangles where tsdf is exactly 0: nothing is welded by
    position or decimated, and color.mesh_colors colours it.  min_weight's default is untested for quality."""
    who = "volume_mesh"
    min_weight = ops._real(who, "min_weight", min_weight, ">= 0", fp32=True)
    M = mesh_matrix(origin, voxel, T)
    nz, ny, nx = ops._volume_planes(who, least=2, tsdf=tsdf, wsum=wsum)
    need = int(_lib.query("ecms_mesh_scratch_bytes", nx, ny, nz))
    if need <= 0:
        raise RuntimeError(f"{who}: a volume of {nz} x {ny} x {nx} points: at most 2^27")
    dev = tsdf.device
    scratch = ops.torch.empty(need, dtype=torch.uint8, device=dev)
    counts = ops.torch.empty(2, dtype=torch.int64, device=dev)
    _lib.call("ecms_mesh_count_fwd", ops._p(tsdf), ops._p(wsum), ops._p(counts), ops._p(scratch), C.c_longlong(need), nx, ny, nz,
              min_weight, ops._stream())
    N, F = (int(v) for v in counts.tolist())                               # the one host synchronisation
    vertices = ops.torch.empty((N, 3), dtype=torch.float32, device=dev)
    faces = ops.torch.empty((F, 3), dtype=torch.int32, device=dev)
    normals = ops.torch.empty((N, 3), dtype=torch.float32, device=dev) if with_normals else None
    weight = ops.torch.empty((N,), dtype=torch.float32, device=dev) if with_weight else None
    if N:
        Md = M.to(dev)
        _lib.call("ecms_mesh_emit_fwd", ops._p(tsdf), ops._p(wsum), ops._p(Md), ops._p(vertices), ops._p(faces), ops._p(normals),
                  ops._p(weight), ops._p(scratch), C.c_longlong(need), C.c_longlong(N), C.c_longlong(F), nx, ny, nz, min_weight,
                  ops._stream())
    return Mesh(vertices, faces, normals, weight)


def _write_ply(path, mesh, colors, who):
    """The one PLY writer, on the host: binary little-endian; per vertex float x y z, float nx ny nz where the mesh has normals,
    and uchar red green blue (alpha) where `colors` ([N,3] or [N,4]; None: no colour) is given; per face `list uchar int
    vertex_indices`.  A colour c is stored as floor(clamp(c, 0, 1) * 255 + 0.5), computed in fp64 (a NaN as 0).  `who` names the
    caller in the refusals."""
    if not isinstance(mesh, Mesh):
        raise ValueError(f"{who}: mesh {type(mesh).__name__}: a Mesh")
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.dim() != 2 or colors.shape[1] not in (3, 4)
                               or colors.shape[0] != mesh.vertices.shape[0]):
        raise ValueError(f"{who}: colors {tuple(getattr(colors, 'shape', ()))!r} against vertices {tuple(mesh.vertices.shape)}: [N,3] or [N,4]")
    v, f = mesh.vertices.detach().cpu().to(torch.float32), mesh.faces.detach().cpu().to(torch.int32)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{who}: vertices {tuple(v.shape)}, faces {tuple(f.shape)}: [N,3] and [F,3]")
    names = ["x", "y", "z"]
    if mesh.normals is not None:
        n = mesh.normals.detach().cpu().to(torch.float32)
        if n.shape != v.shape:
            raise ValueError(f"{who}: normals {tuple(n.shape)} against vertices {tuple(v.shape)}")
        v, names = torch.cat([v, n], 1), names + ["nx", "ny", "nz"]
    fields, channels = [("f", "<f4", (v.shape[1],))], []
    if colors is not None:
        c = torch.nan_to_num(colors.detach().cpu().to(torch.float64), nan=0.0)
        c = torch.floor(c.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
        fields, channels = fields + [("c", "u1", (c.shape[1],))], ["red", "green", "blue", "alpha"][:c.shape[1]]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + [f"property float {n}" for n in names] \
        + [f"property uchar {n}" for n in channels] + [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(v.shape[0], dtype=np.dtype(fields))                    # packed: no padding
    rows["f"] = v.numpy()
    if colors is not None:
        rows["c"] = c.numpy()
    tris = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    tris["n"], tris["i"] = 3, f.numpy()
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(rows.tobytes())
        out.write(tris.tobytes())


def write_ply(path, mesh):
    """Write `mesh` (a Mesh, on any device) to `path` as binary little-endian PLY, on the host: per vertex float x y z and, where
    the mesh has normals, float nx ny nz; per face `list uchar int vertex_indices`.  color.write_ply adds vertex colours."""
    _write_ply(path, mesh, None, "write_ply")
