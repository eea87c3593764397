#!/usr/bin/env python3
"""What the TSDF volume costs: 576 x 960 views of a ramp-and-step scene integrated into volumes of 128^3
and 256^3 voxels, V = 1 and V = 4 views per launch, and the raycast of each volume at 576 x 960.  Per case: the launch of
ecmv_integrate_fwd / ecmv_raycast_fwd alone on preallocated buffers, the op of ops.py with its checks, its host-side matrices
and their one host-to-device copy, the same result computed by ATen on the same device tensors (an fp64 restatement of
include/ecm_volume.h: elementwise planes and gathers; the raycast's march is a Python loop over the samples, so it is given
fewer iterations), and a plain device copy whose rate stands for the streaming ceiling.  The integration must move 16 bytes per
voxel (two fp32 planes read and written); its gathers from the views mostly hit in cache and are not counted.
Device events around each call, medians with the lowest and the highest sample beside them; the sides alternate inside one loop.
Usage: python tools/volume_time.py [--iters 100] [--out profiles/r28_volume_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecm_amd  # noqa: E402

H, W = 576, 960
F64, F32 = torch.float64, torch.float32
TRUNC = 0.3


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


def scene(V):
    """A ramp (the ground) with a step (a box in front of it), shifted by two pixels per view: disparities from 30 to 100 px."""
    y = torch.arange(H, device="cuda", dtype=F32).view(1, H, 1)
    x = torch.arange(W, device="cuda", dtype=F32).view(1, 1, W)
    d = (30.0 + 40.0 * y / H + 0.01 * x).expand(V, H, W).clone()
    for v in range(V):
        d[v, H // 3:2 * H // 3, W // 3 + 2 * v:W // 2 + 2 * v] = 100.0
    return d.contiguous()


def row_of(m, a, b, c):
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3]


def aten_integrate(tsdf, wsum, disp, weight, Q, G, Cm, trunc, max_weight):
    """include/ecm_volume.h's integration in ATen on the device (tests/test_disp_volume_cpu.py::integrate_t without book-keeping)."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    kk, jj, ii = (t.to(F64) for t in torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev), torch.arange(nx, device=dev),
                                                     indexing="ij"))
    X, N = tsdf, wsum
    for v in range(disp.shape[0]):
        Gv, Cv = G[v], Cm[v]
        h3 = row_of(Gv[3], ii, jj, kk)
        u, vv, dv = row_of(Gv[0], ii, jj, kk) / h3, row_of(Gv[1], ii, jj, kk) / h3, row_of(Gv[2], ii, jj, kk) / h3
        px, py = torch.floor(u + 0.5), torch.floor(vv + 0.5)
        ok = torch.isfinite(u) & torch.isfinite(vv) & torch.isfinite(dv) & (dv > 0) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        px, py = torch.where(ok, px, 0.0), torch.where(ok, py, 0.0)
        at = (py * W + px).long().reshape(-1)
        d = disp[v].reshape(-1)[at].view_as(px)
        w = weight[v].reshape(-1)[at].view_as(px)
        fd = d.to(F64)
        P3 = row_of(Q[3], px, py, fd)
        z_meas, z_vox = row_of(Q[2], px, py, fd) / P3, row_of(Cv[2], ii, jj, kk)
        s = z_meas - z_vox
        ok = ok & torch.isfinite(d) & (d > 0) & torch.isfinite(w) & (w > 0) & torch.isfinite(P3) & (P3 != 0) & torch.isfinite(z_meas) \
            & (z_meas > 0) & torch.isfinite(z_vox) & (z_vox > 0) & ~(s < -trunc)
        t = torch.clamp(s / trunc, max=1.0).to(F32)
        Wn = N + w
        X, N = torch.where(ok, (X * N + t * w) / Wn, X), torch.where(ok, torch.clamp(Wn, max=max_weight), N)
    return X, N


def blend(plane, cell, q):
    nz, ny, nx = plane.shape
    flat = plane.reshape(-1)
    base = (cell[2] * ny + cell[1]) * nx + cell[0]
    t = lambda dz, dy, dx: flat[base + (dz * ny + dy) * nx + dx].to(F64)                          # noqa: E731
    a = [[t(dz, dy, 0) + q[0] * (t(dz, dy, 1) - t(dz, dy, 0)) for dy in (0, 1)] for dz in (0, 1)]
    e = [a[dz][0] + q[1] * (a[dz][1] - a[dz][0]) for dz in (0, 1)]
    return e[0] + q[2] * (e[1] - e[0])


def aten_raycast(tsdf, wsum, R, Ri, near, far, step):
    """include/ecm_volume.h's raycast in ATen on the device, one view: every sample of every ray, the box not clipped."""
    nz, ny, nx = tsdf.shape
    dims, dev = (nx, ny, nz), tsdf.device
    ys, xs = (t.to(F64) for t in torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij"))
    hn, hf = [row_of(R[r], xs, ys, near) for r in range(4)], [row_of(R[r], xs, ys, far) for r in range(4)]
    gn, gf = [hn[a] / hn[3] for a in range(3)], [hf[a] / hf[3] for a in range(3)]
    dr = [gf[a] - gn[a] for a in range(3)]
    nd = torch.ceil(torch.sqrt((dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2]) / step)
    done = ~((nd >= 1) & torch.isfinite(nd))
    ndc = torch.where(done, 1.0, nd)
    before, f0, p0 = torch.zeros_like(done), torch.zeros_like(xs), [torch.zeros_like(xs)] * 3
    res = torch.zeros(H, W, device=dev, dtype=F32)
    for m in range(int(ndc.max()) + 1):
        s = m / ndc
        p = [gn[a] + dr[a] * s for a in range(3)]
        c = [torch.floor(p[a]) for a in range(3)]
        ok = ~done & (m <= ndc)
        for a in range(3):
            ok = ok & (c[a] >= 0) & (c[a] <= dims[a] - 2)
        cell = [torch.where(ok, c[a], 0.0).long() for a in range(3)]
        q = [p[a] - c[a] for a in range(3)]
        ok = ok & (blend((wsum > 0).to(F32), cell, [torch.zeros_like(xs)] * 3) > 0)             # the lower corner only ...
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):                                                               # ... and then all eight
                    ok = ok & (wsum.reshape(-1)[(cell[2] + dz) * ny * nx + (cell[1] + dy) * nx + cell[0] + dx] > 0)
        f = blend(tsdf, cell, q)
        pair = ok & before
        hit = pair & (f0 > 0) & (f <= 0)
        al = f0 / (f0 - f)
        ps = [p0[a] + (p[a] - p0[a]) * al for a in range(3)]
        res = torch.where(hit, (row_of(Ri[2], ps[0], ps[1], ps[2]) / row_of(Ri[3], ps[0], ps[1], ps[2])).to(F32), res)
        done = done | hit | (pair & (f0 < 0) & (f > 0))
        before, f0, p0 = ok, f, p
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--aten-raycast-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_volume_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib = ecm_amd.ops, ecm_amd._lib
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None               # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = ops.q_matrix(721.5, 0.54, 0.5 * W + 0.37, 0.5 * H + 0.21)          # d = 389.6 / z: 30 .. 100 px is 13 m .. 3.9 m
    poses = torch.stack([ops.se3_exp(torch.tensor([0.05 * v, -0.02 * v, 0.04 * v, 0.002 * v, -0.003 * v, 0.001 * v], dtype=F64)) for v in range(4)])
    near, far, step = 110.0, 28.0, 0.5
    rows = []
    for n in (128, 256):
        dims = (n, n, n)
        voxel = 12.8 / n
        origin = (-6.4, -6.4, 2.0)                                         # x, y in +-6.4 m, z in 2 .. 14.8 m
        a_buf = torch.randn(4 * n * n * n, device="cuda", generator=g)     # a copy of 16 bytes per voxel read and written: 2 x the volume
        b_buf = torch.empty_like(a_buf)
        for V in (1, 4):
            disp = scene(V)
            weight = 0.5 + torch.rand(V, H, W, device="cuda", generator=g)
            T = poses[:V]
            m = ops.volume_matrices(Q, T, origin, voxel)
            mats = torch.cat([Q.reshape(-1), m.G.reshape(-1), m.C.reshape(-1)]).cuda()
            Qd, Gd, Cd = mats[:16].view(4, 4), mats[16:16 + 16 * V].view(V, 4, 4), mats[16 + 16 * V:].view(V, 4, 4)
            tsdf, wsum = ops.volume_new(dims, "cuda")
            fns = (lambda: lib.call("ecmv_integrate_fwd", p(tsdf), p(wsum), p(disp), None, p(weight), p(mats), p(mats, 128),
                                    p(mats, 128 + 128 * V), 1, n, n, n, V, H, W, TRUNC, 64.0, 0.0, 3e38, st()),
                   lambda: ops.volume_integrate(tsdf, wsum, disp, Q, T, origin, voxel, TRUNC, weight=weight),
                   lambda: aten_integrate(tsdf, wsum, disp, weight, Qd, Gd, Cd, TRUNC, 64.0),
                   lambda: b_buf.copy_(a_buf))
            launch, op, aten, copy = samples(fns, a.iters, a.warmup)
            fresh = ops.volume_new(dims, "cuda")
            want = aten_integrate(*fresh, disp, weight, Qd, Gd, Cd, TRUNC, 64.0)
            got = ops.volume_integrate(*fresh, disp, Q, T, origin, voxel, TRUNC, weight=weight)
            ceiling = 2 * a_buf.numel() * 4 / (copy[0] * 1e-3)
            row = {"op": "integrate", "dims": list(dims), "views": [V, H, W], "touched_voxels": int((got[1] > 0).sum()),
                   "launch_ms": launch, "volume_integrate_ms": op, "aten_ms": aten, "copy_ms": copy, "copy_GBps": round(ceiling / 1e9, 1),
                   "bytes_per_voxel": 16, "share_of_streaming_ceiling": round(16 * n ** 3 / ceiling / (launch[0] * 1e-3), 4),
                   "aten_over_op": round(aten[0] / op[0], 2),
                   # ATen's device kernels may contract a product and a sum into one operation: equal to rounding, not bit for bit
                   "max_difference_to_aten": [float((got[0] - want[0]).abs().max()), float((got[1] - want[1]).abs().max())],
                   "touched_sets_equal_to_aten": bool(torch.equal(got[1] > 0, want[1] > 0))}
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the raycast of what the four views left, from the third pose
        tsdf, wsum = ops.volume_integrate(*ops.volume_new(dims, "cuda"), disp, Q, poses, origin, voxel, TRUNC, weight=weight)
        r = ops.volume_matrices(Q, poses[2], origin, voxel)
        rm = torch.cat([r.R.reshape(-1), r.Rinv.reshape(-1)]).cuda()
        out = torch.empty(1, H, W, device="cuda")
        fns = (lambda: lib.call("ecmv_raycast_fwd", p(tsdf), p(wsum), p(rm), p(rm, 128), 0, p(out), None, n, n, n, 1, H, W, near, far, step,
                                65536, st()),
               lambda: ops.volume_raycast(tsdf, wsum, Q, poses[2], origin, voxel, (H, W), near, far, step))
        launch, op = samples(fns, a.iters, a.warmup)
        aten, = samples((lambda: aten_raycast(tsdf, wsum, rm[:16].view(4, 4), rm[16:].view(4, 4), near, far, step),), a.aten_raycast_iters, 1)
        got = ops.volume_raycast(tsdf, wsum, Q, poses[2], origin, voxel, (H, W), near, far, step)[0, 0]
        want = aten_raycast(tsdf, wsum, rm[:16].view(4, 4), rm[16:].view(4, 4), near, far, step)
        row = {"op": "raycast", "dims": list(dims), "view": [H, W], "step": step, "hits": int((got > 0).sum()), "launch_ms": launch,
               "volume_raycast_ms": op, "aten_ms": aten, "aten_iters": a.aten_raycast_iters, "aten_over_op": round(aten[0] / op[0], 1),
               "max_difference_to_aten": float((got - want).abs().max()), "holes_equal_to_aten": bool(torch.equal(got > 0, want > 0))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del a_buf, b_buf
        torch.cuda.empty_cache()
    res = {"what": "ecmv_integrate_fwd's and ecmv_raycast_fwd's launch alone on preallocated buffers, the op of ops.py with its checks and "
                   "its host-to-device copy of the matrices, the same result by ATen on the same tensors, and a device copy of 16 bytes per "
                   "voxel; each entry [median, lowest, highest] in ms.  The timed integrations run on a volume that the earlier "
                   "iterations have filled; the ATen raycast marches every sample of every ray in a Python loop and is timed over "
                   "aten_iters iterations only",
           "iters": a.iters, "timing": "device events around each call, alternating inside one loop", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
