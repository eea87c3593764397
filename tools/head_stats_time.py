#!/usr/bin/env python3
"""What the per-pixel uncertainty of the heads costs, at 576 x 960 and B = 1 and 4, for cmfsm (eight),
cmfsm_sub_16 (volume) and bilinear_cmf (trilinear): the statistics op of each head family against the plain head ops on the
same tensors (the plain kernels are the previous release's, bit for bit), and model.predict against model.forward in ms per
stereo pair.  Device-event medians; the two sides of each comparison alternate inside one loop.
Usage: python tools/head_stats_time.py [--iters 20] [--out profiles/r11_head_stats_time.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecm_amd  # noqa: E402

H, W, MAXDISP = 576, 960, 192
ARCHS = {"cmfsm": ("eight", 4), "cmfsm_sub_16": ("volume", 16), "bilinear_cmf": ("trilinear", 4)}


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


def head_pair(kind, s, B, g):
    """(plain, stats) callables of one head family on random operands of the architecture's shapes."""
    ops = ecm_amd.ops
    h, w, Dl = H // s, W // s, MAXDISP // s
    R = lambda *sh, sc=1.0: torch.randn(*sh, device="cuda", generator=g) * sc                    # noqa: E731
    c = R(3, B, Dl, h, w, sc=2.0)
    if kind == "eight":
        w9 = torch.softmax(R(B, 9, H, W), 1)
        return (lambda: ops.ecm_aggregate9(ops.softargmin_heads(c), w9, s)), (lambda: ops.ecm_aggregate9_stats(c, w9, s))
    if kind == "volume":
        m5, mt3 = R(B, 5, H, W, sc=0.5), R(B, 3, H, W, sc=0.5)
        return (lambda: ops.volume_mapping(c, m5, mt3, s)), (lambda: ops.volume_mapping_stats(c, m5, mt3, s))
    return (lambda: ops.trilinear_softargmin(c, MAXDISP, H, W)), (lambda: ops.trilinear_softargmin_stats(c, MAXDISP, H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_head_stats_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for arch, (kind, s) in ARCHS.items():
        torch.manual_seed(0)
        model = ecm_amd.get_model(arch).cuda().eval()
        for B in (1, 4):
            with torch.no_grad():
                plain, stats = medians(head_pair(kind, s, B, g), a.iters, a.warmup)
            left = torch.randn(B, 3, H, W, device="cuda", generator=g)
            right = torch.randn(B, 3, H, W, device="cuda", generator=g)
            with torch.no_grad(), ecm_amd.ops.frozen_weights():
                fwd, pred = medians((lambda: model(left, right), lambda: model.predict(left, right)), max(a.iters // 2, 3), 2)
            rows.append({"arch": arch, "head": kind, "B": B, "plain_head_ms": plain, "stats_head_ms": stats,
                         "stats_over_plain": round(stats / plain, 2), "forward_ms_per_pair": round(fwd / B, 3),
                         "predict_ms_per_pair": round(pred / B, 3), "predict_minus_forward_ms_per_pair": round((pred - fwd) / B, 3)})
            print(json.dumps(rows[-1]), flush=True)
        del model
    out = {"what": "head statistics (std, peak, entropy) against the plain heads, and predict against forward, fp32",
           "frame": [H, W], "maxdisp": MAXDISP, "iters": a.iters, "timing": "device events, median, alternating", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
