#!/usr/bin/env python3
"""What the disparity post-filters cost, at 576 x 960 and 384 x 1248, B = 1 and 4: the median kernel at
r = 1, 2, 3 and the bilateral kernel at r = 4 and the largest radius with C = 3 (on preallocated outputs, and through the op with
its allocation), against the same definitions written in ATen on the device -- what a user would otherwise write: an unfold of
the padded planes, a sort (median) or a weighted sum (bilateral) over the window axis -- and against a plain copy of the planes
each kernel reads plus writes, the HBM floor (median: d, valid as a quarter plane, 2 out = 3.25 planes; bilateral with C = 3:
6.25 planes; the copy reads n and writes n, so it moves twice the bytes).  Device-event medians; the sides alternate inside one
loop.
Usage: python tools/disp_filter_time.py [--iters 30] [--out profiles/r14_disp_filter_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecm_amd  # noqa: E402

FRAMES = ((576, 960), (384, 1248))
SIGMA_SPACE, SIGMA_COLOR, CHANNELS = 2.0, 0.25, 3


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


def windows(t, r, fill):
    """[B,c,H,W] -> [B,c,(2r+1)^2,H,W]: the clipped windows, `fill` outside the image."""
    B, c, H, W = t.shape
    k = 2 * r + 1
    return F.unfold(F.pad(t, (r, r, r, r), value=fill), k).view(B, c, k * k, H, W)


def aten_median(d, valid, r):
    """Section 18's masked lower median in torch ops, fp32 on the device."""
    usable = torch.isfinite(d) & (valid != 0)
    win = windows(torch.where(usable, d, float("inf")).unsqueeze(1), r, float("inf"))[:, 0]
    m = torch.isfinite(win).sum(1)
    med = win.sort(1).values.gather(1, ((m - 1) // 2).clamp(min=0).unsqueeze(1))[:, 0]
    return torch.where(m > 0, med, 0.0), m.float()


def aten_bilateral(d, valid, g, r, ss, sc):
    """Section 18's joint bilateral filter in torch ops, fp32 on the device."""
    usable = torch.isfinite(d) & (valid != 0)
    k = 2 * r + 1
    o = torch.arange(-r, r + 1, device=d.device, dtype=d.dtype)
    spatial = (-(o.view(k, 1) ** 2 + o.view(1, k) ** 2) / (2 * ss * ss)).view(1, k * k, 1, 1)
    dw = windows(torch.where(usable, d, 0.0).unsqueeze(1), r, 0.0)[:, 0]
    uw = windows(usable.float().unsqueeze(1), r, 0.0)[:, 0] > 0
    e = spatial - ((windows(g, r, 0.0) - g.unsqueeze(2)) ** 2).sum(1) / (2 * sc * sc)
    w = torch.where(uw & ~torch.isnan(e), torch.exp(e), 0.0)
    sw = w.sum(1)
    return torch.where(sw > 0, (w * dw).sum(1) / sw.clamp(min=1e-30), 0.0), sw


def planes(B, H, W, g):
    """A `filled`-like map: per-row ramps with steps, streaks of zeros (rows and patches without a consistent pixel) and a guide."""
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    d = 40 * torch.rand(B, H, 1, device="cuda", generator=g) + 20 * ((x // 97) % 2) + 0.01 * x
    d = torch.where(torch.rand(B, H, W, device="cuda", generator=g) < 0.1, torch.zeros_like(d), d)
    d[:, ::37] = 0
    guide = torch.rand(B, CHANNELS, H, W, device="cuda", generator=g) * 0.3 + 0.6 * ((x // 97) % 2).view(1, 1, 1, W)
    return d.contiguous(), (d > 0).to(torch.uint8), guide.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_disp_filter_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib = ecm_amd.ops, ecm_amd._lib
    r_max = ops.disp_filter_max_radius("bilateral")
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    rows = []
    for H, W in FRAMES:
        for B in (1, 4):
            d, valid, guide = planes(B, H, W, g)
            out = torch.empty(2, B, H, W, device="cuda")
            n = B * H * W
            for kind, r in [("median", 1), ("median", 2), ("median", 3), ("bilateral", 4), ("bilateral", r_max)]:
                moved = 3.25 if kind == "median" else 3.25 + CHANNELS            # planes read plus written, in fp32 planes
                src = torch.randn(int(moved * n), device="cuda", generator=g)
                dst = torch.empty_like(src)
                with torch.no_grad():
                    if kind == "median":
                        fns = (lambda: lib.call("ecm_disp_median_fwd", p(d), p(valid), p(out), B, H, W, r, st()),
                               lambda: ops.disparity_median(d, valid, r, with_support=True),
                               lambda: aten_median(d, valid, r))
                        want, got = aten_median(d, valid, r), ops.disparity_median(d, valid, r, with_support=True)
                        agree = float((want[0] == got[0]).float().mean())
                    else:
                        fns = (lambda: lib.call("ecm_disp_bilateral_fwd", p(d), p(valid), p(guide), p(out), B, CHANNELS, H, W, r,
                                                SIGMA_SPACE, SIGMA_COLOR, st()),
                               lambda: ops.disparity_bilateral(d, guide, valid, r, SIGMA_SPACE, SIGMA_COLOR, with_weight=True),
                               lambda: aten_bilateral(d, valid, guide, r, SIGMA_SPACE, SIGMA_COLOR))
                        want = aten_bilateral(d, valid, guide, r, SIGMA_SPACE, SIGMA_COLOR)
                        got = ops.disparity_bilateral(d, guide, valid, r, SIGMA_SPACE, SIGMA_COLOR, with_weight=True)
                        agree = float(((want[0] - got[0]).abs() <= 1e-4 * want[0].abs() + 1e-5).float().mean())
                    del want, got
                    kern, op, aten, copy = medians(fns + (lambda: dst.copy_(src),), a.iters, a.warmup)
                row = {"frame": [H, W], "B": B, "filter": kind, "radius": r, "kernel_ms": kern, "op_ms": op, "aten_chain_ms": aten,
                       "copy_ms": copy, "copy_planes": moved, "aten_over_kernel": round(aten / kern, 1),
                       "kernel_over_copy": round(kern / copy, 2), "kernel_GBps": round(moved * n * 4 / kern / 1e6, 1),
                       "agrees_with_aten": round(agree, 6)}
                rows.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
    out = {"what": "ecm_disp_median_fwd / ecm_disp_bilateral_fwd (C = 3) against the ATen restatement of the same definitions "
                   "(unfold, sort or weighted sum) and a copy of the planes each kernel reads plus writes, fp32",
           "sigma_space": SIGMA_SPACE, "sigma_color": SIGMA_COLOR, "iters": a.iters,
           "timing": "device events, median, alternating", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
