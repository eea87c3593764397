#!/usr/bin/env python3
"""What the disparity reprojection costs, at 576 x 960 and 384 x 1248, B = 1 and 4, with every pixel valid
and with about half of them valid.  Per case: the launches alone on preallocated outputs (ecmg_reproject_fwd: one; ecmg_point_cloud_fwd
with three attribute planes: three), ops.disparity_reproject and ops.point_cloud with their allocations (the cloud op ends in its
one host read of N), an ATen restatement of each on the same tensors -- a meshgrid, an fp64 matmul with Q, the division, the
predicate, and for the cloud `nonzero` and a gather -- and a plain device copy, whose rate stands for the streaming ceiling.
Bytes an op must move per pixel: dense 4 in + 12 out = 16; cloud 8 + (12 + 4 C) * share (the disparity read by the count and again
by the emit, and a row per usable pixel); the valid plane, the mask and the gathered attribute reads come on top and are left out
of the denominator, so the shares reported are on the low side.  The shares are taken from the launch times.
Host clock around device synchronisations, medians with the lowest and the highest sample beside them; the sides alternate
inside one loop.
Usage: python tools/disp_reproject_time.py [--iters 100] [--out profiles/r19_disp_reproject_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ecm_amd  # noqa: E402

FRAMES = ((576, 960), (384, 1248))
ATTRS = 3


def samples(fns, iters, warmup):
    """[median, lowest, highest] time in ms of each callable, synchronised before and after, alternating them."""
    times = [[] for _ in fns]
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[j].append((time.perf_counter() - t0) * 1e3)
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def aten_dense(d, Q, valid):
    """The ATen restatement of the dense op: fp64 throughout, three or four full-frame temporaries."""
    B, H, W = d.shape
    y, x = torch.meshgrid(torch.arange(H, device=d.device, dtype=torch.float64), torch.arange(W, device=d.device, dtype=torch.float64),
                          indexing="ij")
    v = torch.stack([x.expand(B, H, W), y.expand(B, H, W), d.double(), torch.ones(B, H, W, device=d.device, dtype=torch.float64)], 1)
    out = torch.matmul(Q.view(1, 4, 4), v.view(B, 4, H * W)).view(B, 4, H, W)
    w = out[:, 3]
    mask = torch.isfinite(d) & (d > 0) & torch.isfinite(w) & (w != 0)
    if valid is not None:
        mask = mask & valid
    xyz = torch.where(mask.unsqueeze(1), out[:, :3] / w.unsqueeze(1), 0.0).float()
    return xyz, mask


def aten_cloud(d, Q, valid, attrs):
    xyz, mask = aten_dense(d, Q, valid)
    b, y, x = mask.nonzero(as_tuple=True)                                  # synchronises
    points = torch.cat([xyz[b, :, y, x], attrs[b, :, y, x]], 1)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=d.device), mask.flatten(1).sum(1).cumsum(0)])
    return points, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_disp_reproject_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from test_disp_reproject_cpu import kernel_constants
    ops, lib = ecm_amd.ops, ecm_amd._lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                            # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for H, W in FRAMES:
        Q = ops.q_matrix(721.5, 0.54, 0.5 * W + 0.37, 0.5 * H + 0.21).cuda()
        for B in (1, 4):
            n = B * H * W
            d = (1.0 + 190.0 * torch.rand(B, H, W, device="cuda", generator=g)).contiguous()
            attrs = torch.rand(B, ATTRS, H, W, device="cuda", generator=g)
            for label, valid in (("all", None), ("half", torch.rand(B, H, W, device="cuda", generator=g) < 0.5)):
                a_buf = torch.randn(8 * n, device="cuda", generator=g)    # 32 B per pixel in, 32 out: one copy moves 64 B per pixel
                b_buf = torch.empty_like(a_buf)
                v8 = None if valid is None else valid.view(torch.uint8)
                xyz, points = torch.empty(B, 3, H, W, device="cuda"), torch.empty(n, 3 + ATTRS, device="cuda")
                offsets = torch.empty(B + 1, device="cuda", dtype=torch.int64)
                nb = lib.query("ecmg_point_cloud_scratch_bytes", B, H, W)
                scratch = torch.empty(nb, device="cuda", dtype=torch.uint8)
                fns = (lambda: lib.call("ecmg_reproject_fwd", p(d), p(v8), p(Q), 0, p(xyz), None, B, H, W, 0.0, 3e38, st()),
                       lambda: lib.call("ecmg_point_cloud_fwd", p(d), p(v8), p(Q), 0, p(attrs), ATTRS, p(points), p(offsets), None, None,
                                        p(scratch), C.c_longlong(nb), B, H, W, 0.0, 3e38, st()),
                       lambda: ops.disparity_reproject(d, Q, valid, with_mask=True),
                       lambda: ops.point_cloud(d, Q, attrs, valid),
                       lambda: aten_dense(d, Q, valid),
                       lambda: aten_cloud(d, Q, valid, attrs),
                       lambda: b_buf.copy_(a_buf))
                dense_launch, cloud_launch, dense, cloud, a_dense, a_cloud, copy = samples(fns, a.iters, a.warmup)
                points, offsets = ops.point_cloud(d, Q, attrs, valid)
                want_points, want_offsets = aten_cloud(d, Q, valid, attrs)
                share = len(points) / n
                same = torch.equal(offsets, want_offsets) and torch.equal(points[:, 3:], want_points[:, 3:])
                worst = float((points[:, :3] - want_points[:, :3]).abs().max()) if len(points) else 0.0
                ceiling = 2 * a_buf.numel() * 4 / (copy[0] * 1e-3)                       # bytes per second of the copy
                dense_bytes = n * 16
                cloud_bytes = n * (8 + (12 + 4 * ATTRS) * share)
                row = {"frame": [H, W], "B": B, "valid": label, "share": round(share, 4), "attributes": ATTRS,
                       "dense_launch_ms": dense_launch, "cloud_launches_ms": cloud_launch, "dense_ms": dense, "cloud_ms": cloud,
                       "aten_dense_ms": a_dense, "aten_cloud_ms": a_cloud, "copy_ms": copy,
                       "copy_GBps": round(ceiling / 1e9, 1),
                       "dense_share_of_ceiling": round(dense_bytes / ceiling / (dense_launch[0] * 1e-3), 4),
                       "cloud_share_of_ceiling": round(cloud_bytes / ceiling / (cloud_launch[0] * 1e-3), 4),
                       "aten_dense_over_dense": round(a_dense[0] / dense[0], 2), "aten_cloud_over_cloud": round(a_cloud[0] / cloud[0], 2),
                       "order_and_attributes_equal_aten": same, "worst_coordinate_difference_to_aten": worst}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del a_buf, b_buf
                torch.cuda.empty_cache()
    res = {"what": "the launches alone on preallocated outputs (dense: one; cloud with 3 attribute planes: count, scan, emit), "
                   "ops.disparity_reproject (xyz and mask) and ops.point_cloud (with the host read of N), both with their allocations, an ATen restatement of each on the same tensors (fp64 matmul, "
                   "nonzero, gather) and a device copy of 32 B per pixel; each entry [median, lowest, highest] in ms. "
                   "share_of_ceiling = (the bytes the op must move: dense 16 B/pixel, cloud 8 + (12 + 4 C) * share B/pixel) / "
                   "(the copy's bytes per second) / (the median time of the launches alone)",
           "kernel_constants": kernel_constants(), "iters": a.iters,
           "timing": "host clock around device synchronisations, alternating inside one loop", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
