#!/usr/bin/env python3
"""The bf16 encoder (ops.encoder_dtype) in ONE process.

1. Eval forward ms per pair under frozen_weights(): fp32, aggregation-only bf16, and encoder + aggregation bf16, for cmfsm at
   batch 1 and 4 and cmfsm_sub_16 at batch 1 (576x960).
2. Launch tables of the encoder alone (cmfsm's feature_extraction on the 2B = 8 images of a batch-4 forward, 576x960) in fp32
   and in bf16: every launch timed by entry point and shape, and each bf16 convolution's rate in direct-form FLOPs against the
   bf16 dense MFMA peak.

Usage: python tools/bf16_encoder_time.py [--steps N] [--warmup W]  -> JSON lines, then the two tables."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import ecm_amd  # noqa: E402
from bf16_infer_time import MFMA_BF16_PEAK, model_of, timed  # noqa: E402

BF = torch.bfloat16


def forward(model, left, right, enc, agg):
    ops = ecm_amd.ops
    with torch.no_grad(), (ops.encoder_dtype(BF) if enc else contextlib.nullcontext()), \
            (ops.aggregation_dtype(BF) if agg else contextlib.nullcontext()):
        return model(left, right)


def launch_table(fe, x, enc, steps):
    lib = ecm_amd._lib
    ctx = ecm_amd.ops.encoder_dtype(BF) if enc else contextlib.nullcontext()
    with torch.no_grad(), ecm_amd.ops.frozen_weights(), ctx:
        for _ in range(2):
            fe(x)
        torch.cuda.synchronize()
        lib.enable_all_timers()
        for _ in range(steps):
            fe(x)
        torch.cuda.synchronize()
        rec = lib.disable_timers()
    rows, total = [], 0.0
    for name, calls in rec.items():
        groups = {}
        for s, e, ints in calls:
            groups.setdefault(tuple(ints), []).append(s.elapsed_time(e))
        for ints, ts in groups.items():
            ms = sum(ts) / steps
            total += ms
            flop = 0.0
            if name == "ecm_conv2d_bf16_fwd":
                b_, ci, co, h, w, k, st = ints[:7]
                flop = 2.0 * b_ * ci * co * k * k * ((h - 1) // st + 1) * ((w - 1) // st + 1)
            rows.append((name, ints, len(ts) // steps, ms, ms / (len(ts) / steps), flop))
    rows.sort(key=lambda r: -r[3])
    print(f"\nencoder {'bf16' if enc else 'fp32'} (cmfsm feature_extraction, {x.shape[0]} images {x.shape[2]}x{x.shape[3]}): "
          f"launches timed one by one, sum {total:.2f} ms per forward")
    print(f"{'entry point':30s} {'int args':44s} {'n':>3s} {'ms/fwd':>8s} {'ms/call':>8s} {'TFLOP/s':>8s} {'of bf16 peak':>12s}")
    for name, ints, n, ms, per, flop in rows:
        tf = flop / (per * 1e-3) / 1e12 if flop else 0.0
        pk = f"{flop / (per * 1e-3) / MFMA_BF16_PEAK:12.1%}" if flop else ""
        print(f"{name:30s} {str(tuple(ints))[:44]:44s} {n:3d} {ms:8.3f} {per:8.3f} {tf:8.1f} {pk}")
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator(device="cpu").manual_seed(1234)
    for arch, B, H, W in (("cmfsm", 1, 576, 960), ("cmfsm", 4, 576, 960), ("cmfsm_sub_16", 1, 576, 960)):
        model = model_of(arch)
        left, right = torch.randn(B, 3, H, W, generator=g).cuda(), torch.randn(B, 3, H, W, generator=g).cuda()
        with ecm_amd.ops.frozen_weights():
            f32 = timed(lambda: forward(model, left, right, False, False), a.steps, a.warmup)
            agg = timed(lambda: forward(model, left, right, False, True), a.steps, a.warmup)
            both = timed(lambda: forward(model, left, right, True, True), a.steps, a.warmup)
        print(json.dumps({"arch": arch, "B": B, "hw": [H, W], "fp32_ms_per_pair": round(f32 / B, 2),
                          "agg_bf16_ms_per_pair": round(agg / B, 2), "enc_agg_bf16_ms_per_pair": round(both / B, 2),
                          "speedup_vs_fp32": round(f32 / both, 3), "speedup_vs_agg_only": round(agg / both, 3)}), flush=True)
        del model, left, right
    fe = model_of("cmfsm").feature_extraction
    x = torch.randn(8, 3, 576, 960, generator=g).cuda()
    t32 = launch_table(fe, x, False, a.steps)
    t16 = launch_table(fe, x, True, a.steps)
    print(json.dumps({"encoder_launch_sum_ms": {"fp32": round(t32, 2), "bf16": round(t16, 2)}}))


if __name__ == "__main__":
    main()
