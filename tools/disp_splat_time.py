#!/usr/bin/env python3
"""What the disparity splat costs, at 576 x 960 and 384 x 1248, B = 1 and 4: the one launch of
ecm_disp_splat_fwd on preallocated outputs (right and src), ops.disparity_splat with its allocations, and a plain device copy of
the planes the launch reads plus writes (one in, two out: the HBM floor, as in sections 18-20).  The copy reads n and writes n, so
it moves twice its size.  With --model also cmfsm at 576 x 960, B = 1: forward, cross_check, self_check, and smooth as it is
(two forwards: the existing path, the baseline) and inside models.occlusion_check("splat").
Device-event medians with the lowest and the highest sample beside them; the sides alternate inside one loop.
Usage: python tools/disp_splat_time.py [--iters 200] [--model] [--out profiles/r17_disp_splat_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ecm_amd  # noqa: E402

FRAMES = ((576, 960), (384, 1248))
PLANES = 3                                    # d in, right and src out


def samples(fns, iters, warmup):
    """[median, lowest, highest] device time in ms of each callable, alternating them."""
    times = [[] for _ in fns]
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            if i >= warmup:
                times[j].append(s.elapsed_time(e))
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def disparity_like(B, H, W, g):
    """Per-row ramps with steps of 20 px every 97 columns and 0.3 px of noise: occlusion bands, ties nowhere."""
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    d = 40 * torch.rand(B, H, 1, device="cuda", generator=g) + 20 * ((x // 97) % 2) + 0.01 * x
    return (d + 0.3 * torch.randn(B, H, W, device="cuda", generator=g)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_disp_splat_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from test_disp_splat_cpu import kernel_constants, splat_t
    ops, lib = ecm_amd.ops, ecm_amd._lib
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    rows = []
    for H, W in FRAMES:
        for B in (1, 4):
            n = B * H * W
            d = disparity_like(B, H, W, g)
            right, src = torch.empty(B, H, W, device="cuda"), torch.empty(B, H, W, device="cuda", dtype=torch.int32)
            a_buf = torch.randn(PLANES * n // 2, device="cuda", generator=g)
            b_buf = torch.empty_like(a_buf)
            fns = (lambda: lib.call("ecm_disp_splat_fwd", p(d), p(right), p(src), B, H, W, st()),
                   lambda: ops.disparity_splat(d, with_source=True),
                   lambda: b_buf.copy_(a_buf))
            launch, op, copy = samples(fns, a.iters, a.warmup)
            want_right, want_src = splat_t(d.cpu())
            got_right, got_src = ops.disparity_splat(d, with_source=True)
            same = torch.equal(got_right.cpu().view(torch.int32), want_right.view(torch.int32)) and torch.equal(got_src.cpu().long(), want_src)
            kind = ops.lr_check(d, got_right)[1]
            row = {"frame": [H, W], "B": B, "launch_ms": launch, "op_ms": op, "copy_ms": copy, "copy_planes": PLANES,
                   "launch_over_copy": round(launch[0] / copy[0], 2), "bit_identical_to_splat_t": same,
                   "holes": round(float((got_src < 0).float().mean()), 4), "occluded": round(float((kind == 1).float().mean()), 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del a_buf, b_buf
            torch.cuda.empty_cache()
    res = {"what": "ecm_disp_splat_fwd (one launch: an LDS integer-max splat of each row and its decode) on preallocated outputs, "
                   "ops.disparity_splat with its allocations, and a copy of the planes the launch reads plus writes; each entry "
                   "[median, lowest, highest] in ms",
           "kernel_constants": kernel_constants(), "iters": a.iters,
           "timing": "device events, alternating inside one loop", "rows": rows}
    if a.model:
        H, W = FRAMES[0]
        model = ecm_amd.get_model("cmfsm").cuda().eval()
        left, right_img = (torch.randn(1, 3, H, W, device="cuda", generator=g) for _ in range(2))
        iters = max(a.iters // 4, 10)

        def smooth_splat():
            with ecm_amd.models.occlusion_check("splat"):
                return model.smooth(left, right_img)

        with torch.no_grad():
            fwd, cc, sc, cross, splat = samples((lambda: model(left, right_img), lambda: model.cross_check(left, right_img),
                                                 lambda: model.self_check(left, right_img),
                                                 lambda: model.smooth(left, right_img), smooth_splat), iters, 3)
        res["model"] = {"frame": [H, W], "B": 1, "arch": "cmfsm", "iters": iters, "input": "seeded normal noise, random weights",
                        "forward_ms": fwd, "cross_check_ms": cc, "self_check_ms": sc, "smooth_cross_ms": cross, "smooth_splat_ms": splat,
                        "smooth_splat_over_cross": round(splat[0] / cross[0], 4),
                        "self_check_minus_forward_ms": round(sc[0] - fwd[0], 3),
                        "smooth_splat_minus_forward_ms": round(splat[0] - fwd[0], 3)}
        print(json.dumps(res["model"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
