#!/usr/bin/env python3
"""What the mesh of the TSDF volume costs: volumes of 128^3 and 256^3 points holding the three-plane scene of
tests/test_motion_align_cpu.py (four 240 x 384 views integrated by ops.volume_integrate) and a sphere.  Per case: the two entries
ecms_mesh_count_fwd and ecms_mesh_emit_fwd alone on preallocated buffers, the whole op mesh.volume_mesh (its checks, its matrix,
its allocations and the host synchronisation between the two entries), a plain device copy of the 8 bytes per point that the
count pass must read, and an ATen restatement on the same tensors of PART of the work -- usable and live flags, the seven slot
planes, the vertex count, the triangle count and the vertex positions, without normals, weights or face indices -- so the ratio
to the op is a lower bound.  Device events around each call, medians with the lowest and the highest sample beside them; the
sides alternate inside one loop.
Usage: python tools/mesh_time.py [--iters 100] [--out profiles/r31_mesh_time.json]"""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ecm_amd  # noqa: E402

F64, F32 = torch.float64, torch.float32
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
H, W = 240, 384


def samples(fns, iters, warmup):
    """[median, lowest, highest] time in ms of each callable between two device events, alternating them."""
    times = [[] for _ in fns]
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            e.synchronize()
            if i >= warmup:
                times[j].append(s.elapsed_time(e))
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def planes_volume(n):
    """The three planes at about 3 m, seen from four poses, in a box of 3.2 m: (tsdf, wsum, origin, voxel)."""
    from test_disp_volume_cpu import VIEWS
    from test_motion_align_cpu import PLANES, render, scene_q
    ops = ecm_amd.ops
    Q = scene_q(H, W)
    disp = torch.stack([render(p, H, W, PLANES, Q).to(F32) for p in VIEWS]).cuda()
    voxel = 3.2 / (n - 1)
    origin = (-1.6, -1.6, 1.5)
    tsdf, wsum = ops.volume_integrate(*ops.volume_new((n, n, n), "cuda"), disp, Q, torch.stack(VIEWS), origin, voxel, 6 * voxel)
    return tsdf, wsum, origin, voxel


def sphere_volume(n):
    c = (n - 1) / 2
    k, j, i = torch.meshgrid(*[torch.arange(n, device="cuda", dtype=F32)] * 3, indexing="ij")
    r = torch.sqrt((i - c) ** 2 + (j - c) ** 2 + (k - c) ** 2)
    return ((r - 0.3 * n) / 4.0).clamp(-1, 1).contiguous(), torch.ones(n, n, n, device="cuda"), (-1.6, -1.6, 1.5), 3.2 / (n - 1)


def shifted(a, d, fill):
    """a at p + d (d = (dx, dy, dz), each 0 or +-1), `fill` outside the grid."""
    out = torch.full_like(a, fill)
    n = a.shape
    src = tuple(slice(max(s, 0), m + min(s, 0)) for s, m in zip(d[::-1], n))
    dst = tuple(slice(max(-s, 0), m + min(-s, 0)) for s, m in zip(d[::-1], n))
    out[dst] = a[src]
    return out


def aten_part(tsdf, wsum, M, min_weight=0.0):
    """(N, F, vertices [N,3] fp32) of include/ecm_mesh.h in ATen on the device."""
    nz, ny, nx = tsdf.shape
    usable = (wsum > min_weight) & torch.isfinite(tsdf)
    pos = tsdf > 0
    live = torch.zeros_like(usable)
    lv = torch.ones((nz - 1, ny - 1, nx - 1), dtype=torch.bool, device=tsdf.device)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        lv &= usable[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    live[:nz - 1, :ny - 1, :nx - 1] = lv
    has = []
    for dr in DIRS:
        within = torch.zeros_like(usable)
        for back in itertools.product(*[(0,) if v else (0, 1) for v in dr]):
            within |= shifted(live, tuple(-b for b in back), False)
        has.append((pos != shifted(pos, dr, False)) & within)
    has = torch.stack(has, -1)
    kk, jj, ii, dd = torch.nonzero(has, as_tuple=True)
    dr = torch.tensor(DIRS, device=tsdf.device)[dd]
    t0, t1 = tsdf[kk, jj, ii].to(F64), tsdf[kk + dr[:, 2], jj + dr[:, 1], ii + dr[:, 0]].to(F64)
    a = t0 / (t0 - t1)
    g = [ii + dr[:, 0] * a, jj + dr[:, 1] * a, kk + dr[:, 2] * a]
    vertices = torch.stack([(((M[r, 0] * g[0] + M[r, 1] * g[1]) + M[r, 2] * g[2]) + M[r, 3]).to(F32) for r in range(3)], 1)
    # the triangles: per tetrahedron one for one or three positive corners, two for two
    F = 0
    corner = lambda o: shifted(pos, o, False)                                                    # noqa: E731
    for perm in itertools.permutations(range(3)):
        c1 = [0, 0, 0]
        c1[perm[0]] = 1
        c2 = list(c1)
        c2[perm[1]] = 1
        k = pos.to(torch.int32) + corner(tuple(c1)) + corner(tuple(c2)) + corner((1, 1, 1))
        F += int((torch.where(k == 2, 2, ((k == 1) | (k == 3)).to(torch.int32)) * live).sum())
    return len(ii), F, vertices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--aten-iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_mesh_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib, mesh = ecm_amd.ops, ecm_amd._lib, ecm_amd.mesh
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                            # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    rows = []
    for n in (128, 256):
        src = torch.randn(2 * n ** 3, device="cuda")                       # 8 bytes per point
        dst = torch.empty_like(src)
        for scene, build in (("three planes", planes_volume), ("sphere", sphere_volume)):
            tsdf, wsum, origin, voxel = build(n)
            need = lib.query("ecms_mesh_scratch_bytes", n, n, n)
            scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
            counts = torch.zeros(2, dtype=torch.int64, device="cuda")
            count = lambda: lib.call("ecms_mesh_count_fwd", p(tsdf), p(wsum), p(counts), p(scratch), C.c_longlong(need), n, n, n, 0.0, st())   # noqa: E731
            count()
            N, F = counts.tolist()
            M = mesh.mesh_matrix(origin, voxel)
            Md = M.cuda()
            vertices, normals = torch.empty(N, 3, device="cuda"), torch.empty(N, 3, device="cuda")
            faces = torch.empty(F, 3, dtype=torch.int32, device="cuda")
            emit = lambda: lib.call("ecms_mesh_emit_fwd", p(tsdf), p(wsum), p(Md), p(vertices), p(faces), p(normals), None, p(scratch),   # noqa: E731
                                    C.c_longlong(need), C.c_longlong(N), C.c_longlong(F), n, n, n, 0.0, st())
            t_count, t_emit, t_op, t_copy = samples((count, emit, lambda: mesh.volume_mesh(tsdf, wsum, origin, voxel), lambda: dst.copy_(src)),
                                                    a.iters, a.warmup)
            t_aten, = samples((lambda: aten_part(tsdf, wsum, Md),), a.aten_iters, 1)
            aN, aF, av = aten_part(tsdf, wsum, Md)
            got = mesh.volume_mesh(tsdf, wsum, origin, voxel)
            row = {"scene": scene, "dims": [n, n, n], "N": N, "F": F, "count_ms": t_count, "emit_ms": t_emit, "volume_mesh_ms": t_op,
                   "copy_8_bytes_per_point_ms": t_copy, "copy_GBps": round(2 * 8 * n ** 3 / (t_copy[0] * 1e-3) / 1e9, 1),
                   "count_over_copy": round(t_count[0] / t_copy[0], 2), "aten_part_ms": t_aten, "aten_iters": a.aten_iters,
                   "aten_part_over_op": round(t_aten[0] / t_op[0], 1), "counts_equal_to_aten": [aN == N, aF == F],
                   # ATen's device kernels may contract a product and a sum into one operation: equal to rounding, not bit for bit
                   "max_vertex_difference_to_aten": float((got.vertices - av).abs().max()) if N else 0.0}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del scratch, vertices, normals, faces, got, av
        del src, dst
        torch.cuda.empty_cache()
    res = {"what": "ecms_mesh_count_fwd and ecms_mesh_emit_fwd alone on preallocated buffers, mesh.volume_mesh with its checks, allocations "
                   "and its one host synchronisation, a device copy of 8 bytes per point (read and written: twice the bytes the count pass "
                   "must read), and ATen on the same tensors for the flags, the counts and the vertex positions only; each entry "
                   "[median, lowest, highest] in ms",
           "iters": a.iters, "timing": "device events around each call, alternating inside one loop", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
