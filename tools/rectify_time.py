#!/usr/bin/env python3
"""What stereo rectification costs: 1080 x 1920 uint8 raw frames to 576 x 960 network inputs through the
maps of a synthetic rig (about one degree of rotation about each axis, five distortion coefficients), B = 1 and 4.  Per case: the
remap launch alone on preallocated outputs (ecmr_remap_pair_fwd, both views, no image, no masks), ops.remap_pair with its
allocations, the map launch alone (ecmr_rectify_map_fwd, one view) and ops.rectify_map, an ATen restatement of the remap on the
same tensors -- uint8 HWC to float CHW, grid_sample(bilinear, zeros, align_corners=True) on a normalised grid built once outside
the timed region, then (s / 255 - mean) / std, for both views -- and a plain device copy, whose rate stands for the streaming
ceiling.  Bytes the remap must move: both raw frames once (2 * 3 B per source pixel: an upper bound, the maps of this rig touch
most of the frame), the outputs (2 * 12 B per output pixel) and the two shared maps once (2 * 8 B per output pixel, not per
image).  The share is taken from the launch time.
Host clock around device synchronisations, medians with the lowest and the highest sample beside them; the sides alternate inside
one loop.
Usage: python tools/rectify_time.py [--iters 100] [--out profiles/r20_rectify_time.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecm_amd  # noqa: E402

RAW, NET = (1080, 1920), (576, 960)


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


def synthetic_rig():
    H, W = RAW
    K1 = torch.tensor([[1400.0, 0, 0.5 * W + 7.3], [0, 1398.0, 0.5 * H - 4.1], [0, 0, 1]], dtype=torch.float64)
    K2 = torch.tensor([[1405.0, 0, 0.5 * W - 5.2], [0, 1402.0, 0.5 * H + 6.4], [0, 0, 1]], dtype=torch.float64)
    D1 = torch.tensor([-0.17, 0.06, 0.0008, -0.0005, -0.01], dtype=torch.float64)
    D2 = torch.tensor([-0.16, 0.05, -0.0006, 0.0009, 0.008], dtype=torch.float64)
    a = math.radians(1.0)
    R = ecm_amd.ops._rotation_matrix(torch.tensor([a, -0.8 * a, 0.6 * a], dtype=torch.float64))
    T = torch.tensor([-0.54, 0.004, -0.006], dtype=torch.float64)
    return ecm_amd.models.StereoRig(K1, D1, K2, D2, R, T, RAW, new_size=NET), (K1, D1)


def aten_grid(mp, H, W):
    """[1,Ho,Wo,2] normalised coordinates of a map [2,Ho,Wo] for grid_sample(align_corners=True)."""
    return torch.stack([mp[0] * (2.0 / (W - 1)) - 1.0, mp[1] * (2.0 / (H - 1)) - 1.0], -1).unsqueeze(0)


def aten_remap(raw_l, raw_r, grid_l, grid_r, mean, std):
    out = []
    for raw, grid in ((raw_l, grid_l), (raw_r, grid_r)):
        src = raw.permute(0, 3, 1, 2).float()
        s = torch.nn.functional.grid_sample(src, grid.expand(raw.shape[0], -1, -1, -1), mode="bilinear", padding_mode="zeros",
                                            align_corners=True)
        out.append((s / 255.0 - mean) / std)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_rectify_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib = ecm_amd.ops, ecm_amd._lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                            # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    host = lambda v: C.cast((C.c_float * 3)(*v), C.c_void_p)                                     # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    rig, (K1, D1) = synthetic_rig()
    ml, mr = rig.maps("cuda")
    (H, W), (Ho, Wo) = RAW, NET
    r = rig.rectification
    params = ops.rectify_map_params(K1, D1, r.R1, r.P1).cuda()
    map_out = torch.empty(2, Ho, Wo, device="cuda")
    grid_l, grid_r = aten_grid(ml, H, W), aten_grid(mr, H, W)
    mean = torch.tensor(ops.FLYING3D_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(ops.FLYING3D_STD, device="cuda").view(1, 3, 1, 1)
    m3, s3 = host(ops.FLYING3D_MEAN), host(ops.FLYING3D_STD)
    rows = []
    for B in (1, 4):
        # smooth frames (an upsampled random field): neighbouring taps differ little, as in a photograph
        low = torch.rand(2 * B, 3, H // 8, W // 8, device="cuda", generator=g)
        raw = (torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear") * 255).round().to(torch.uint8)
        raw_l, raw_r = (t.permute(0, 2, 3, 1).contiguous() for t in (raw[:B], raw[B:]))
        left, right = torch.empty(B, 3, Ho, Wo, device="cuda"), torch.empty(B, 3, Ho, Wo, device="cuda")
        n_copy = 16 * B * Ho * Wo                                             # floats: 64 B per output pixel in, 64 out
        a_buf = torch.randn(n_copy, device="cuda", generator=g)
        b_buf = torch.empty_like(a_buf)
        fns = (lambda: lib.call("ecmr_remap_pair_fwd", p(raw_l), p(raw_r), 1, p(ml), p(mr), 0, p(left), p(right), None, None, None,
                                B, H, W, Ho, Wo, m3, s3, 0.0, st()),
               lambda: ops.remap_pair(raw_l, raw_r, ml, mr),
               lambda: ops.remap_pair(raw_l, raw_r, ml, mr, want_image=True, with_mask=True),
               lambda: lib.call("ecmr_rectify_map_fwd", p(params), p(map_out), Ho, Wo, st()),
               lambda: ops.rectify_map(K1, D1, r.R1, r.P1, NET, "cuda"),
               lambda: aten_remap(raw_l, raw_r, grid_l, grid_r, mean, std),
               lambda: b_buf.copy_(a_buf))
        launch, op, op_all, map_launch, map_op, aten, copy = samples(fns, a.iters, a.warmup)
        got = ops.remap_pair(raw_l, raw_r, ml, mr, with_mask=True)
        want = aten_remap(raw_l, raw_r, grid_l, grid_r, mean, std)
        inside = got[2] & got[3]                                              # grid_sample rounds its coordinates differently at the rim
        worst = max(float(((gt - w) * k.unsqueeze(1)).abs().max()) for gt, w, k in ((got[0], want[0], got[2]), (got[1], want[1], got[3])))
        ceiling = 2 * a_buf.numel() * 4 / (copy[0] * 1e-3)                    # bytes per second of the copy
        moved = B * (2 * 3 * H * W + 2 * 12 * Ho * Wo) + 2 * 8 * Ho * Wo
        row = {"raw": [H, W], "net": [Ho, Wo], "B": B, "remap_launch_ms": launch, "remap_pair_ms": op,
               "remap_pair_image_masks_ms": op_all, "map_launch_ms": map_launch, "rectify_map_ms": map_op, "aten_remap_ms": aten,
               "copy_ms": copy, "copy_GBps": round(ceiling / 1e9, 1), "bytes_moved": moved,
               "remap_GBps": round(moved / (launch[0] * 1e-3) / 1e9, 1),
               "remap_share_of_ceiling": round(moved / ceiling / (launch[0] * 1e-3), 4),
               "aten_over_remap_pair": round(aten[0] / op[0], 2), "inside_share": round(float(inside.float().mean()), 4),
               "worst_difference_to_aten_inside": worst}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del a_buf, b_buf
        torch.cuda.empty_cache()
    res = {"what": "the remap launch alone on preallocated outputs (both views, uint8 HWC source, shared maps, no image, no masks), "
                   "ops.remap_pair with its allocations (plain, and with the image and both masks), the map launch alone and "
                   "ops.rectify_map (one view), an ATen restatement of the remap on the same tensors (uint8 -> float CHW, grid_sample "
                   "on a grid built outside the timed region, the normalisation; both views) and a device copy of 64 B per output "
                   "pixel; each entry [median, lowest, highest] in ms.  share_of_ceiling = bytes_moved / (the copy's bytes per "
                   "second) / (the median launch time); bytes_moved = B * (2 * 3 * H * W + 2 * 12 * Ho * Wo) + 2 * 8 * Ho * Wo",
           "tile_width": ops.rectify_tile_width(), "iters": a.iters,
           "timing": "host clock around device synchronisations, alternating inside one loop", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
