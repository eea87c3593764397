#!/usr/bin/env python3
"""What the speckle filter costs, at 576 x 960 and 384 x 1248, B = 1 and 4: the whole launch sequence of
ecm_disp_speckle_fwd on preallocated outputs, and ops.disparity_speckle with its allocations, on three inputs --
  disparity   a disparity-like map (per-row ramps with steps and 0.3 px of noise) with 10 % invalid;
  constant    one value, everything valid: one segment per image, the worst contention on one root;
  serpentine  a one-pixel-wide path through every other row, the rest invalid: one segment with the longest paths --
against a plain copy of the planes the sequence reads plus writes, the HBM floor as in section 18 (local: d, a quarter for the
byte mask, label and size out; count: label and size in, out out; emit: out and d in, label, size and out out = 11.25 planes, the merge's
border pixels and the root look-ups not counted; the copy reads n and writes n, so it moves twice the bytes).  There is no ATen
formulation to compare with.  Device-event medians; the sides alternate inside one loop.
Usage: python tools/disp_speckle_time.py [--iters 30] [--out profiles/r15_disp_speckle_time.json]"""
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

FRAMES = ((576, 960), (384, 1248))
MAX_SIZE, MAX_DIFF, PLANES = 200, 1.0, 11.25


def medians(fns, iters, warmup):
    """Median device time in ms of each callable, alternating them."""
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
    return [round(statistics.median(t), 4) for t in times]


def inputs(B, H, W, g):
    """name -> (d, valid)."""
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    d = 40 * torch.rand(B, H, 1, device="cuda", generator=g) + 20 * ((x // 97) % 2) + 0.01 * x
    d = (d + 0.3 * torch.randn(B, H, W, device="cuda", generator=g)).contiguous()
    valid = (torch.rand(B, H, W, device="cuda", generator=g) >= 0.1).to(torch.uint8)
    path = torch.zeros(H, W, dtype=torch.uint8, device="cuda")
    path[0::2] = 1
    path[1::4, W - 1] = 1
    path[3::4, 0] = 1
    const = torch.full((B, H, W), 17.5, device="cuda")
    return {"disparity": (d, valid), "constant": (const, torch.ones_like(valid)),
            "serpentine": (const, path.view(1, H, W).expand(B, H, W).contiguous())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_disp_speckle_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib = ecm_amd.ops, ecm_amd._lib
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    rows = []
    for H, W in FRAMES:
        for B in (1, 4):
            n = B * H * W
            out, seg = torch.empty(B, H, W, device="cuda"), torch.empty(2, B, H, W, device="cuda", dtype=torch.int32)
            src = torch.randn(int(PLANES * n), device="cuda", generator=g)
            dst = torch.empty_like(src)
            base = None
            for name, (d, valid) in inputs(B, H, W, g).items():
                fns = (lambda: lib.call("ecm_disp_speckle_fwd", p(d), p(valid), p(out), p(seg), B, H, W, MAX_SIZE, MAX_DIFF, st()),
                       lambda: ops.disparity_speckle(d, valid, MAX_SIZE, MAX_DIFF, with_segments=True),
                       lambda: dst.copy_(src))
                kept, _, size = ops.disparity_speckle(d, valid, MAX_SIZE, MAX_DIFF, with_segments=True)
                stats = {"usable": round(float((size > 0).float().mean()), 4), "largest_segment": int(size.max()),
                         "removed": round(float(((size > 0) & (size <= MAX_SIZE)).float().mean()), 4)}
                del kept, size
                seq, op, copy = medians(fns, a.iters, a.warmup)
                base = seq if name == "disparity" else base
                row = {"frame": [H, W], "B": B, "input": name, "sequence_ms": seq, "op_ms": op, "copy_ms": copy,
                       "copy_planes": PLANES, "sequence_over_copy": round(seq / copy, 2),
                       "sequence_over_disparity_input": round(seq / base, 2), "sequence_GBps": round(PLANES * n * 4 / seq / 1e6, 1),
                       **stats}
                rows.append(row)
                print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    res = {"what": "ecm_disp_speckle_fwd (four launches: local, merge, count, emit) against a copy of the planes the sequence reads "
                   "plus writes, fp32, on a disparity-like map with 10 % invalid, a constant plane and a one-pixel serpentine",
           "max_size": MAX_SIZE, "max_diff": MAX_DIFF, "iters": a.iters, "timing": "device events, median, alternating", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
