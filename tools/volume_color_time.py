#!/usr/bin/env python3
"""What colour in the TSDF volume costs, on tools/volume_time.py's scene: 576 x 960 views integrated into
128^3 and 256^3 voxels, V = 1 and V = 4, with A = 3 attribute planes.  Per case the launch of ecmc_integrate_fwd alone on
preallocated buffers beside ecmv_integrate_fwd on the same volume (the geometry alone; with --parent-lib also the entry of a
library built from the commit before this one), beside ecmv_integrate_fwd followed by a separate colour pass's floor (a device copy
of the (A + 1) * 4 bytes per voxel that pass would read and write), and beside a device copy of all (2 + A + 1) * 4 bytes per
voxel; the raycast of each volume at 576 x 960 beside ecmv_raycast_fwd; the point sampling at 100 000 and 330 000 points; and a
ColorStereoMapper frame beside a StereoMapper frame.  Device events around each call, medians with the lowest and the highest
sample beside them; the sides alternate inside one loop.
Usage: python tools/volume_color_time.py [--iters 100] [--out profiles/r32_volume_color_time.json] [--parent-lib lib.so]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ecm_amd  # noqa: E402
from volume_time import F32, F64, H, TRUNC, W, samples, scene  # noqa: E402

A = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_volume_color_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib, color, models = ecm_amd.ops, ecm_amd._lib, ecm_amd.color, ecm_amd.models
    parent = None
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        res, args = lib.VOLUME_PROTOTYPES["ecmv_integrate_fwd"]
        parent.ecmv_integrate_fwd.restype, parent.ecmv_integrate_fwd.argtypes = res, args
        res, args = lib.VOLUME_PROTOTYPES["ecmv_raycast_fwd"]
        parent.ecmv_raycast_fwd.restype, parent.ecmv_raycast_fwd.argtypes = res, args
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None               # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = ops.q_matrix(721.5, 0.54, 0.5 * W + 0.37, 0.5 * H + 0.21)
    poses = torch.stack([ops.se3_exp(torch.tensor([0.05 * v, -0.02 * v, 0.04 * v, 0.002 * v, -0.003 * v, 0.001 * v], dtype=F64)) for v in range(4)])
    near, far, step = 110.0, 28.0, 0.5
    rows = []
    for n in (128, 256):
        dims = (n, n, n)
        voxel, origin = 12.8 / n, (-6.4, -6.4, 2.0)
        P = n ** 3
        all_a, all_b = torch.randn((2 + A + 1) * P, device="cuda", generator=g), torch.empty((2 + A + 1) * P, device="cuda")
        col_a, col_b = all_a[:(A + 1) * P], all_b[:(A + 1) * P]
        for V in (1, 4):
            disp = scene(V)
            weight = 0.5 + torch.rand(V, H, W, device="cuda", generator=g)
            attrs = torch.rand(V, A, H, W, device="cuda", generator=g)
            T = poses[:V]
            m = ops.volume_matrices(Q, T, origin, voxel)
            mats = torch.cat([Q.reshape(-1), m.G.reshape(-1), m.C.reshape(-1)]).cuda()
            tsdf, wsum = ops.volume_new(dims, "cuda")
            attr, asum = color.volume_attributes_new(dims, A, "cuda")
            t2, w2 = ops.volume_new(dims, "cuda")
            geometry = (p(disp), None, p(weight), p(mats), p(mats, 128), p(mats, 128 + 128 * V), 1, n, n, n, V, H, W, TRUNC, 64.0, 0.0, 3e38)
            fns = [lambda: lib.call("ecmc_integrate_fwd", p(tsdf), p(wsum), p(attr), p(asum), p(disp), None, p(weight), p(attrs), p(mats),
                                    p(mats, 128), p(mats, 128 + 128 * V), 1, n, n, n, A, V, H, W, TRUNC, 64.0, 0.0, 3e38, st()),
                   lambda: lib.call("ecmv_integrate_fwd", p(t2), p(w2), *geometry, st()),
                   lambda: all_b.copy_(all_a),
                   lambda: col_b.copy_(col_a),
                   lambda: color.volume_integrate(tsdf, wsum, attr, asum, disp, attrs, Q, T, origin, voxel, TRUNC, weight=weight)]
            if parent is not None:
                t3, w3 = ops.volume_new(dims, "cuda")
                fns.append(lambda: parent.ecmv_integrate_fwd(p(t3), p(w3), *geometry, st()))
            got = samples(fns, a.iters, a.warmup)
            fused, geo, copy_all, copy_col, op = got[:5]
            # the timed volumes have seen different numbers of calls: compare one call each from an empty volume
            for t in (tsdf, t2):
                t.fill_(1.0)
            for t in (wsum, w2, attr, asum):
                t.zero_()
            fns[0](), fns[1]()
            if parent is not None:
                t3.fill_(1.0), w3.zero_()
                fns[5]()
            row = {"op": "integrate", "dims": list(dims), "views": [V, H, W], "A": A, "coloured_voxels": int((asum > 0).sum()),
                   "touched_voxels": int((wsum > 0).sum()), "ecmc_integrate_fwd_ms": fused, "ecmv_integrate_fwd_ms": geo,
                   "copy_all_planes_ms": copy_all, "copy_colour_planes_ms": copy_col, "color_volume_integrate_ms": op,
                   "bytes_per_voxel": (2 + A + 1) * 4, "fused_over_geometry": round(fused[0] / geo[0], 3),
                   "fused_over_copy_of_all_planes": round(fused[0] / copy_all[0], 3),
                   "geometry_plus_colour_pass_floor_ms": round(geo[0] + copy_col[0], 4),
                   "tsdf_wsum_bit_equal_to_ecmv": bool(torch.equal(tsdf.view(torch.int32), t2.view(torch.int32))
                                                       and torch.equal(wsum.view(torch.int32), w2.view(torch.int32)))}
            if parent is not None:
                row["parent_ecmv_integrate_fwd_ms"] = got[5]
                row["tsdf_wsum_bit_equal_to_parent"] = bool(torch.equal(t2.view(torch.int32), t3.view(torch.int32))
                                                            and torch.equal(w2.view(torch.int32), w3.view(torch.int32)))
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the raycast of what four views left, from the third pose
        vol = color.volume_integrate(*ops.volume_new(dims, "cuda"), *color.volume_attributes_new(dims, A, "cuda"), disp, attrs, Q, poses, origin,
                                     voxel, TRUNC, weight=weight)
        r = ops.volume_matrices(Q, poses[2], origin, voxel)
        rm = torch.cat([r.R.reshape(-1), r.Rinv.reshape(-1)]).cuda()
        out, out2, out3 = (torch.empty(1, H, W, device="cuda") for _ in range(3))
        cols = torch.empty(1, A, H, W, device="cuda")
        tail = (n, n, n, 1, H, W, near, far, step, 65536)
        fns = [lambda: lib.call("ecmc_raycast_fwd", p(vol[0]), p(vol[1]), p(vol[2]), p(vol[3]), p(rm), p(rm, 128), 0, p(out), None, p(cols), n, n, n,
                                A, 1, H, W, near, far, step, 65536, st()),
               lambda: lib.call("ecmv_raycast_fwd", p(vol[0]), p(vol[1]), p(rm), p(rm, 128), 0, p(out2), None, *tail, st()),
               lambda: color.volume_raycast(*vol, Q, poses[2], origin, voxel, (H, W), near, far, step)]
        if parent is not None:
            fns.append(lambda: parent.ecmv_raycast_fwd(p(vol[0]), p(vol[1]), p(rm), p(rm, 128), 0, p(out3), None, *tail, st()))
        got = samples(fns, a.iters, a.warmup)
        row = {"op": "raycast", "dims": list(dims), "view": [H, W], "A": A, "step": step, "hits": int((out > 0).sum()),
               "ecmc_raycast_fwd_ms": got[0], "ecmv_raycast_fwd_ms": got[1], "color_volume_raycast_ms": got[2],
               "colour_over_geometry": round(got[0][0] / got[1][0], 3),
               "out_bit_equal_to_ecmv": bool(torch.equal(out.view(torch.int32), out2.view(torch.int32)))}
        if parent is not None:
            row["parent_ecmv_raycast_fwd_ms"] = got[3]
            row["out_bit_equal_to_parent"] = bool(torch.equal(out2.view(torch.int32), out3.view(torch.int32)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if n == 256:
            for N in (100000, 330000):
                lo = torch.tensor(origin, device="cuda", dtype=F32)
                pts = lo + 12.8 * torch.rand(N, 3, device="cuda", generator=g)
                Minv = torch.linalg.inv(ecm_amd.mesh.mesh_matrix(origin, voxel)).contiguous().cuda()
                o = torch.empty(N, A, device="cuda")
                launch, op = samples([lambda: lib.call("ecmc_sample_fwd", p(vol[2]), p(vol[3]), p(Minv), p(pts), p(o), C.c_longlong(N), n, n, n, A,
                                                       st()),
                                      lambda: color.volume_sample(vol[2], vol[3], pts, origin, voxel)], a.iters, a.warmup)
                row = {"op": "sample", "dims": list(dims), "points": N, "A": A, "ecmc_sample_fwd_ms": launch, "color_volume_sample_ms": op,
                       "coloured_points": int((o != 0).any(1).sum())}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del all_a, all_b, col_a, col_b, vol
        torch.cuda.empty_cache()
    # one frame of the mapper, the motion given: the network, the tracker and one integration
    hw = (256, 512)
    model = ecm_amd.get_model("cmfsm").cuda().eval()
    frames = [torch.randn(1, 3, *hw, device="cuda", generator=g) for _ in range(2)]
    Qm = ops.q_matrix(700.0, 0.25, 0.5 * hw[1], 0.5 * hw[0])
    motion = ops.se3_exp(torch.tensor([0.002, -0.003, 0.001, 0.01, 0.0, -0.05], dtype=F64))
    args = (model, Qm, (-2.0, -1.0, 0.5), 0.03125, (128, 64, 128), 0.25)
    mappers = (models.ColorStereoMapper(*args, min_disp=0.5), models.StereoMapper(*args, min_disp=0.5))
    with torch.no_grad():
        got = samples([lambda m=m: m(frames[0], frames[1], motion=motion) for m in mappers], a.frames, 2)
    row = {"op": "mapper frame", "frame": list(hw), "dims": [128, 64, 128], "channels": 3, "ColorStereoMapper_ms": got[0], "StereoMapper_ms": got[1],
           "frames": a.frames}
    rows.append(row)
    print(json.dumps(row), flush=True)
    res = {"what": "launches alone on preallocated buffers, ops with their checks and host-to-device copies, and device copies of the "
                   "planes' bytes; each entry [median, lowest, highest] in ms.  The timed integrations run on a volume that the earlier "
                   "iterations have filled.  parent_*: the same entry of a library built from the commit before this one",
           "iters": a.iters, "timing": "device events around each call, alternating inside one loop", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
