#!/usr/bin/env python3
"""What the left-right consistency check costs, at 576 x 960 and 384 x 1248, B = 1 and 4: the one
kernel behind ops.lr_check (on preallocated outputs, and through the op with its allocation) against the torch/ATen
restatement of the same definitions run on the device -- what a user would otherwise write: a flip, two gathers, the
compares, a cummax and a cummin, three more gathers -- and against a plain copy of 5 planes, the HBM floor (the kernel reads
2 planes and writes 3; the copy reads 5 and writes 5).  Device-event medians; the sides alternate inside one loop.
Usage: python tools/lr_check_time.py [--iters 50] [--out profiles/r13_lr_check_time.json]"""
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
THRESHOLD, REL = 1.0, 0.05


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


def aten_lr_check(dl, dr_mirrored, threshold, rel):
    """The definitions of section 17 in torch ops, fp32 on the device; dr as forward(flip(right), flip(left)) returns it."""
    W = dl.shape[-1]
    dr = dr_mirrored.flip(2)
    idx = torch.arange(W, device=dl.device).expand(dl.shape)
    xr = idx.to(dl.dtype) - dl
    oov = ~torch.isfinite(dl) | (xr < 0) | (xr > W - 1)
    xs = torch.where(oov, torch.zeros_like(xr), xr)
    f = xs.floor()
    x0 = f.long()
    r0, r1 = dr.gather(2, x0), dr.gather(2, (x0 + 1).clamp(max=W - 1))
    r = r0 + (xs - f) * (r1 - r0)
    rfin = torch.isfinite(r)
    error = torch.where(oov | ~rfin, torch.full_like(dl, float("inf")), (dl - r).abs())
    cons = ~oov & (error <= (rel * dl).clamp(min=threshold))
    kind = torch.where(oov, 3.0, torch.where(cons, 0.0, torch.where(rfin & (r > dl), 1.0, 2.0)))
    Lx = torch.where(cons, idx, -1).cummax(2).values
    Rx = torch.where(cons, idx, W).flip(2).cummin(2).values.flip(2)
    hl, hr = Lx >= 0, Rx < W
    a, b = dl.gather(2, Lx.clamp(min=0)), dl.gather(2, Rx.clamp(max=W - 1))
    src = torch.where(cons, idx, torch.where(hr & (~hl | (b < a)), Rx, Lx))
    filled = torch.where(src >= 0, dl.gather(2, src.clamp(min=0)), torch.zeros_like(dl))
    return error, kind, filled


def planes(B, H, W, g):
    """A left ramp per row with steps (objects) and the right view it implies, mirrored, plus noise: every kind occurs."""
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    a = 40 * torch.rand(B, H, 1, device="cuda", generator=g)
    dl = a + 20 * ((x // 97) % 2) + 0.01 * x
    dr = dl + (torch.rand(B, H, W, device="cuda", generator=g) * 4 - 2)
    return dl.contiguous(), dr.flip(2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_lr_check_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib = ecm_amd.ops, ecm_amd._lib
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    rows = []
    for H, W in FRAMES:
        for B in (1, 4):
            dl, dr = planes(B, H, W, g)
            check = torch.empty(3, B, H, W, device="cuda")
            five, five_out = torch.randn(5, B, H, W, device="cuda", generator=g), torch.empty(5, B, H, W, device="cuda")
            want = aten_lr_check(dl, dr, THRESHOLD, REL)
            got = ops.lr_check(dl, dr, THRESHOLD, REL, mirrored=True)
            kinds = [round(float((got[1] == k).float().mean()), 4) for k in range(4)]
            agree = round(float((got[1] == want[1]).float().mean()), 6)
            with torch.no_grad():
                kern, op, aten, copy = medians((
                    lambda: lib.call("ecm_lr_check_fwd", p(dl), p(dr), p(check), C.c_void_p(0), B, H, W, THRESHOLD, REL, 1, st()),
                    lambda: ops.lr_check(dl, dr, THRESHOLD, REL, mirrored=True),
                    lambda: aten_lr_check(dl, dr, THRESHOLD, REL),
                    lambda: five_out.copy_(five)), a.iters, a.warmup)
            row = {"frame": [H, W], "B": B, "kernel_ms": kern, "op_ms": op, "aten_chain_ms": aten, "copy_5_planes_ms": copy,
                   "aten_over_kernel": round(aten / kern, 1), "kernel_over_copy": round(kern / copy, 2),
                   "kernel_GBps": round(5 * B * H * W * 4 / kern / 1e6, 1), "kind_shares": kinds, "kind_agrees_with_aten": agree}
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"what": "ecm_lr_check_fwd (mirrored, no src plane) against the ATen restatement of the same definitions and a copy of "
                   "5 planes, fp32", "threshold": THRESHOLD, "rel": REL, "iters": a.iters,
           "timing": "device events, median, alternating", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
