#!/usr/bin/env python3
"""fp32 against bf16 aggregation (ops.aggregation_dtype) in ONE process: eval forward ms per pair of cmfsm at batch 1 and 4
(576x960) and of one /16 architecture (cmfsm_sub_16) at 576x960 (at 384x1248 its 1/16 volume is 78 wide, which the
hourglass cannot halve twice and double back: the fp32 model refuses it too), under frozen_weights() (packed layouts cached, as an
evaluation loop would run it).  With --kernels, every launch of one bf16 cmfsm forward (batch 4, 576x960) is timed by entry
point, and each bf16 convolution's rate is set against the bf16 dense MFMA peak in direct-form FLOPs.

Usage: python tools/bf16_infer_time.py [--steps N] [--warmup W] [--kernels]  -> JSON lines (and a table with --kernels)."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ecm_amd  # noqa: E402
from oracle.weights import tensor_for  # noqa: E402

MFMA_BF16_PEAK = 16 * 157.3e12   # flop/s dense: v_mfma_f32_32x32x16_bf16 runs 16x the fp32 MFMA rate


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def model_of(arch):
    m = ecm_amd.get_model(arch)
    m.load_state_dict({k: tensor_for(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().eval()


def forward(model, left, right, bf16):
    ctx = ecm_amd.ops.aggregation_dtype(torch.bfloat16) if bf16 else contextlib.nullcontext()
    with torch.no_grad(), ctx:
        return model(left, right)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cpu").manual_seed(1234)
    for arch, B, H, W in (("cmfsm", 1, 576, 960), ("cmfsm", 4, 576, 960), ("cmfsm_sub_16", 1, 576, 960)):
        model = model_of(arch)
        left, right = torch.randn(B, 3, H, W, generator=g).cuda(), torch.randn(B, 3, H, W, generator=g).cuda()
        with ecm_amd.ops.frozen_weights():
            f32 = timed(lambda: forward(model, left, right, False), a.steps, a.warmup)
            b16 = timed(lambda: forward(model, left, right, True), a.steps, a.warmup)
        print(json.dumps({"arch": arch, "B": B, "hw": [H, W], "fp32_ms_per_pair": round(f32 / B, 2),
                          "bf16_ms_per_pair": round(b16 / B, 2), "speedup": round(f32 / b16, 3)}), flush=True)
        del model, left, right
    if not a.kernels:
        return
    # ---- every launch of one bf16 forward (cmfsm, B=4, 576x960), grouped by entry point and shape
    lib = ecm_amd._lib
    model = model_of("cmfsm")
    B, H, W = 4, 576, 960
    left, right = torch.randn(B, 3, H, W, generator=g).cuda(), torch.randn(B, 3, H, W, generator=g).cuda()
    with ecm_amd.ops.frozen_weights():
        for _ in range(2):
            forward(model, left, right, True)
        torch.cuda.synchronize()
        lib.enable_all_timers()
        for _ in range(a.steps):
            forward(model, left, right, True)
        torch.cuda.synchronize()
        rec = lib.disable_timers()
    rows, total = [], 0.0
    for name, calls in rec.items():
        groups = {}
        for s, e, ints in calls:
            groups.setdefault(tuple(ints), []).append(s.elapsed_time(e))
        for ints, ts in groups.items():
            ms = sum(ts) / a.steps
            total += ms
            flop = 0.0
            if name == "ecm_conv3d_k3_bf16_fwd":
                b_, ci, co, d, h, w, st = ints
                flop = 2.0 * b_ * ci * co * 27 * ((d - 1) // st + 1) * ((h - 1) // st + 1) * ((w - 1) // st + 1)
            elif name == "ecm_deconv3d_k3s2_bf16_fwd":
                b_, ci, co, d, h, w = ints
                flop = 2.0 * b_ * ci * co * 27 * d * h * w
            per = ms / (len(ts) / a.steps)
            rows.append((name, ints, len(ts) // a.steps, ms, per, flop))
    rows.sort(key=lambda r: -r[3])
    print(f"bf16 cmfsm forward B={B} {H}x{W}: launches timed one by one (sum {total:.2f} ms per forward, incl. the fp32 encoder)")
    print(f"{'entry point':32s} {'int args':34s} {'n':>3s} {'ms/fwd':>8s} {'ms/call':>8s} {'TFLOP/s':>8s} {'of bf16 peak':>12s}")
    for name, ints, n, ms, per, flop in rows:
        if ms < 0.05:
            continue
        tf = flop / (per * 1e-3) / 1e12 if flop else 0.0
        pk = f"{flop / (per * 1e-3) / MFMA_BF16_PEAK:12.1%}" if flop else ""
        print(f"{name:32s} {str(ints)[:34]:34s} {n:3d} {ms:8.3f} {per:8.3f} {tf:8.1f} {pk}")


if __name__ == "__main__":
    main()
