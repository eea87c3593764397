#!/usr/bin/env python3
"""What the WLS smoother costs, at 576 x 960 and 384 x 1248, B = 1 and 4, T = 3, C = 3: the 2T launches of
ecm_disp_wls_fwd on preallocated outputs, ops.disparity_wls with its allocations, a plain device copy of the planes the sequence
reads plus writes (the HBM floor, as in sections 18 and 19), and wls_t -- the ATen restatement of tests/test_disp_wls_cpu.py --
on the device (once: its column loop takes seconds).  With --model also model.smooth on cmfsm against its two forwards.
Planes per pass: N, D in, c', N', D' out, the same three back in, N, D out = 10, plus 2C guide planes in (each value is read as
a pixel and as its neighbour's neighbour) = 16 at C = 3; 2T passes.  The copy reads n and writes n, so it moves twice its size.
Device-event medians; the sides alternate inside one loop.
Usage: python tools/disp_wls_time.py [--iters 30] [--model] [--out profiles/r16_disp_wls_time.json]"""
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
LAM, SIGMA, T, CH = 8000.0, 0.25, 3, 3
PLANES = 2 * T * (10 + 2 * CH)


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
    """(d, guide, conf): a disparity-like map (per-row ramps with steps and 0.3 px of noise), an image-like guide with edges at the
    steps, and a 0/1 confidence with 15 % holes in bands."""
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    band = (x // 97) % 2
    d = 40 * torch.rand(B, H, 1, device="cuda", generator=g) + 20 * band + 0.01 * x
    d = (d + 0.3 * torch.randn(B, H, W, device="cuda", generator=g)).contiguous()
    guide = (0.1 * torch.randn(B, CH, H, W, device="cuda", generator=g) + band.view(1, 1, 1, W)).contiguous()
    conf = ((torch.rand(B, H, W, device="cuda", generator=g) >= 0.05) & ((x % 97) >= 10)).float().contiguous()
    return d, guide, conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_disp_wls_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from test_disp_wls_cpu import kernel_constants, wls_t
    ops, lib = ecm_amd.ops, ecm_amd._lib
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    rows = []
    for H, W in FRAMES:
        for B in (1, 4):
            n = B * H * W
            d, guide, conf = inputs(B, H, W, g)
            out = torch.empty(2, B, H, W, device="cuda")
            scratch = torch.empty(lib.query("ecm_disp_wls_scratch_bytes", B, H, W), dtype=torch.uint8, device="cuda")
            src = torch.randn(PLANES * n // 2, device="cuda", generator=g)
            dst = torch.empty_like(src)
            fns = (lambda: lib.call("ecm_disp_wls_fwd", p(d), p(conf), p(guide), p(out), p(scratch), B, CH, H, W, LAM, SIGMA, T, st()),
                   lambda: ops.disparity_wls(d, guide, conf, LAM, SIGMA, T, with_weight=True),
                   lambda: dst.copy_(src))
            seq, op, copy = medians(fns, a.iters, a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = wls_t(d, guide, conf, LAM, SIGMA, T)
            torch.cuda.synchronize()
            aten = round((time.perf_counter() - t0) * 1e3, 1)
            got = ops.disparity_wls(d, guide, conf, LAM, SIGMA, T)
            row = {"frame": [H, W], "B": B, "sequence_ms": seq, "per_pass_ms": round(seq / (2 * T), 4), "op_ms": op, "copy_ms": copy,
                   "copy_planes": PLANES, "sequence_over_copy": round(seq / copy, 2), "aten_wls_t_ms": aten,
                   "aten_over_sequence": round(aten / seq, 1), "max_abs_diff_to_aten_px": float((got - ref[0]).abs().max()),
                   "ns_per_position_of_a_line": round(seq * 1e6 / (T * 2 * (H + W)), 1),
                   "confident": round(float(conf.mean()), 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del src, dst, ref, got
            torch.cuda.empty_cache()
    res = {"what": "ecm_disp_wls_fwd (2T launches: a row pass and a column pass per iteration, forward and backward sweep in one "
                   "kernel) against a copy of the planes the sequence reads plus writes and against wls_t in ATen on the device; "
                   "ns_per_position_of_a_line = sequence / (T * 2 * (H + W)): the time per step of the dependent chain if the two "
                   "sweeps of a pass were all a pass did",
           "lam": LAM, "sigma_color": SIGMA, "iterations": T, "C": CH, "kernel_constants": kernel_constants(), "iters": a.iters,
           "timing": "device events, median, alternating; wls_t: wall clock of one run", "rows": rows}
    if a.model:
        model = ecm_amd.get_model("cmfsm").cuda().eval()
        res["model"] = []
        for H, W in FRAMES:
            left, right = (torch.randn(1, 3, H, W, device="cuda", generator=g) for _ in range(2))
            with torch.no_grad():
                fwd, cc, smooth = medians((lambda: model(left, right), lambda: model.cross_check(left, right),
                                           lambda: model.smooth(left, right)), max(a.iters // 3, 5), 2)
            row = {"frame": [H, W], "B": 1, "arch": "cmfsm", "forward_ms": fwd, "cross_check_ms": cc, "smooth_ms": smooth,
                   "smooth_minus_two_forwards_ms": round(smooth - 2 * fwd, 3),
                   "share_not_forwards": round((smooth - 2 * fwd) / smooth, 4), "smooth_minus_cross_check_ms": round(smooth - cc, 3)}
            res["model"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
