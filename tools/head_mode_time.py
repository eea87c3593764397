#!/usr/bin/env python3
"""What the modal disparity of the heads costs, at 576 x 960 and B = 1 and 4, for cmfsm (eight),
cmfsm_sub_16 (volume) and bilinear_cmf (trilinear): per head family the plain head op, the statistics op and the mode op on
the same tensors, for the eight head also its two mixture kernels alone on the same stored normalisers (aggregate9_stats_fwd,
one thread per pixel and 864 exponentials each, against the LDS-staged aggregate9_mode_fwd), and model.predict() against
model.predict(mode_radius=8) in ms per stereo pair.  Device-event medians; the sides of each comparison alternate inside one loop.
Usage: python tools/head_mode_time.py [--iters 20] [--out profiles/r12_head_mode_time.json]"""
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

H, W, MAXDISP, RADIUS = 576, 960, 192, 8
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


def head_ops(kind, s, B, g):
    """(plain, stats, mode) callables of one head family on random operands of the architecture's shapes, and for the eight head
    the (stats kernel, mode kernel) pair alone."""
    ops, lib = ecm_amd.ops, ecm_amd._lib
    h, w, Dl = H // s, W // s, MAXDISP // s
    R = lambda *sh, sc=1.0: torch.randn(*sh, device="cuda", generator=g) * sc                    # noqa: E731
    c = R(3, B, Dl, h, w, sc=2.0)
    if kind == "eight":
        w9 = torch.softmax(R(B, 9, H, W), 1)
        d, lse, out = torch.empty(3, B, h, w, device="cuda"), torch.empty(3, B, h, w, device="cuda"), torch.empty(3, 3, B, H, W, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())                                                   # noqa: E731
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                         # noqa: E731
        hs = C.c_longlong(B * Dl * h * w)
        lib.call("ecm_softargmin_heads_lse_fwd", p(c), hs, p(d), p(lse), 3, B, Dl, h * w, st())
        kernels = (lambda: lib.call("ecm_aggregate9_stats_fwd", p(c), hs, p(lse), p(w9), p(out), 3, B, Dl, h, w, s, st()),
                   lambda: lib.call("ecm_aggregate9_mode_fwd", p(c), hs, p(lse), p(w9), p(out), 3, B, Dl, h, w, s, RADIUS, st()))
        return ((lambda: ops.ecm_aggregate9(ops.softargmin_heads(c), w9, s)), (lambda: ops.ecm_aggregate9_stats(c, w9, s)),
                (lambda: ops.ecm_aggregate9_mode(c, w9, s, RADIUS))), kernels
    if kind == "volume":
        m5, mt3 = R(B, 5, H, W, sc=0.5), R(B, 3, H, W, sc=0.5)
        return ((lambda: ops.volume_mapping(c, m5, mt3, s)), (lambda: ops.volume_mapping_stats(c, m5, mt3, s)),
                (lambda: ops.volume_mapping_mode(c, m5, mt3, s, RADIUS))), None
    return ((lambda: ops.trilinear_softargmin(c, MAXDISP, H, W)), (lambda: ops.trilinear_softargmin_stats(c, MAXDISP, H, W)),
            (lambda: ops.trilinear_softargmin_mode(c, MAXDISP, H, W, RADIUS))), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_head_mode_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for arch, (kind, s) in ARCHS.items():
        torch.manual_seed(0)
        model = ecm_amd.get_model(arch).cuda().eval()
        for B in (1, 4):
            fns, kernels = head_ops(kind, s, B, g)
            with torch.no_grad():
                plain, stats, mode = medians(fns, a.iters, a.warmup)
            row = {"arch": arch, "head": kind, "B": B, "radius": RADIUS, "plain_head_ms": plain, "stats_head_ms": stats,
                   "mode_head_ms": mode, "mode_over_plain": round(mode / plain, 2)}
            if kernels:
                ks, km = medians(kernels, a.iters, a.warmup)
                row.update({"aggregate9_stats_kernel_ms": ks, "aggregate9_mode_kernel_ms": km, "stats_kernel_over_mode_kernel": round(ks / km, 1)})
            left = torch.randn(B, 3, H, W, device="cuda", generator=g)
            right = torch.randn(B, 3, H, W, device="cuda", generator=g)
            with torch.no_grad(), ecm_amd.ops.frozen_weights():
                pred, modal = medians((lambda: model.predict(left, right), lambda: model.predict(left, right, mode_radius=RADIUS)),
                                      max(a.iters // 2, 3), 2)
            row.update({"predict_ms_per_pair": round(pred / B, 3), "predict_mode_ms_per_pair": round(modal / B, 3),
                        "mode_minus_predict_ms_per_pair": round((modal - pred) / B, 3)})
            rows.append(row)
            print(json.dumps(row), flush=True)
        del model
    out = {"what": "modal disparity (mode, mass, index) against the plain and the statistics heads, and predict(mode_radius=8) "
                   "against predict(), fp32", "frame": [H, W], "maxdisp": MAXDISP, "radius": RADIUS, "iters": a.iters,
           "timing": "device events, median, alternating", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
