#!/usr/bin/env python3
"""The bf16 refinement decoder (ops.decoder_dtype) in ONE process.

1. cmf eval forward ms per pair at 576x960, batch 1 and 4, under frozen_weights(): fp32, aggregation bf16, encoder +
   aggregation bf16, and all three regions bf16 (ops.inference_dtype).
2. The decoder alone (super_resolution_refinement on the 3B = 12 image shapes of a batch-4 forward), fp32 against bf16.
3. Launch tables of the decoder alone in fp32 and in bf16: every launch timed by entry point and shape; the bf16
   convolutions' rate in direct-form FLOPs against the bf16 dense MFMA peak, conv_out's in bytes moved per second.

Usage: python tools/bf16_decoder_time.py [--steps N] [--warmup W]  -> JSON lines, then the two tables."""
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
MODES = {"fp32": (False, False, False), "agg": (False, True, False), "enc_agg": (True, True, False), "all": (True, True, True)}


def region(enc, agg, dec):
    ops = ecm_amd.ops
    st = contextlib.ExitStack()
    st.enter_context(torch.no_grad())
    for on, scope in ((enc, ops.encoder_dtype), (agg, ops.aggregation_dtype), (dec, ops.decoder_dtype)):
        if on:
            st.enter_context(scope(BF))
    return st


def work(name, ints):
    """-> (flop, bytes) of a decoder launch, from its integer arguments."""
    if name == "ecm_conv2d_bf16_fwd":
        b, ci, co, h, w, k, st = ints[:7]
        return 2.0 * b * ci * co * k * k * ((h - 1) // st + 1) * ((w - 1) // st + 1), 0.0
    if name == "ecm_deconv2d_k3s2_bias_bf16_fwd":
        b, ci, co, h, w = ints[:5]
        return 2.0 * b * ci * co * 9 * h * w, 2.0 * b * h * w * (ci + 4 * co)
    if name == "ecm_conv2d_c1_bf16_fwd":
        b, ci, h, w = ints[:4]
        return 2.0 * b * ci * 9 * h * w, b * h * w * (2.0 * ci + 4.0)
    return 0.0, 0.0


def launch_table(srr, ins, dec, steps):
    lib = ecm_amd._lib
    with region(False, False, dec), ecm_amd.ops.frozen_weights():
        for _ in range(2):
            srr(*ins)
        torch.cuda.synchronize()
        lib.enable_all_timers()
        for _ in range(steps):
            srr(*ins)
        torch.cuda.synchronize()
        rec = lib.disable_timers()
    rows, total = [], 0.0
    for name, calls in rec.items():
        groups = {}
        for s, e, ints in calls:
            groups.setdefault(tuple(ints) + tuple(ints.longs), []).append(s.elapsed_time(e))
        for ints, ts in groups.items():
            ms = sum(ts) / steps
            total += ms
            rows.append((name, ints, len(ts) // steps, ms, ms / (len(ts) / steps)) + work(name, ints))
    rows.sort(key=lambda r: -r[3])
    print(f"\ndecoder {'bf16' if dec else 'fp32'} (super_resolution_refinement, {ins[0].shape[0] * ins[0].shape[1]} images "
          f"{ins[1].shape[2]}x{ins[1].shape[3]}): launches timed one by one, sum {total:.2f} ms per forward")
    print(f"{'entry point':34s} {'int args':44s} {'n':>3s} {'ms/fwd':>8s} {'ms/call':>8s} {'TFLOP/s':>8s} {'of bf16 peak':>12s} {'TB/s':>6s}")
    for name, ints, n, ms, per, flop, nbytes in rows:
        tf = f"{flop / (per * 1e-3) / 1e12:8.1f}" if flop else " " * 8
        pk = f"{flop / (per * 1e-3) / MFMA_BF16_PEAK:12.1%}" if flop and name != "ecm_conv2d_c1_bf16_fwd" else " " * 12
        tb = f"{nbytes / (per * 1e-3) / 1e12:6.2f}" if nbytes else ""
        print(f"{name:34s} {str(tuple(ints))[:44]:44s} {n:3d} {ms:8.3f} {per:8.3f} {tf} {pk} {tb}")
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator(device="cpu").manual_seed(1234)
    H, W = 576, 960
    model = model_of("cmf")
    for B in (1, 4):
        left, right = torch.randn(B, 3, H, W, generator=g).cuda(), torch.randn(B, 3, H, W, generator=g).cuda()
        out = {"arch": "cmf", "B": B, "hw": [H, W]}
        with ecm_amd.ops.frozen_weights():
            for mode, flags in MODES.items():
                def fwd():
                    with region(*flags):
                        return model(left, right)
                out[mode + "_ms_per_pair"] = round(timed(fwd, a.steps, a.warmup) / B, 2)
        out["all_vs_enc_agg"] = round(out["enc_agg_ms_per_pair"] / out["all_ms_per_pair"], 3)
        out["all_vs_fp32"] = round(out["fp32_ms_per_pair"] / out["all_ms_per_pair"], 3)
        print(json.dumps(out), flush=True)
        del left, right
    srr, B, h, w = model.srr, 4, H // 4, W // 4
    ins = ((torch.rand(3, B, h, w, generator=g) * 48.0).cuda(), torch.randn(B, 3, H, W, generator=g).cuda(),
           torch.randn(B, 32, h, w, generator=g).cuda(), torch.randn(B, 32, 2 * h, 2 * w, generator=g).cuda())
    alone = {}
    with ecm_amd.ops.frozen_weights():
        for dec in (False, True):
            def run():
                with region(False, False, dec):
                    return srr(*ins)
            alone["bf16" if dec else "fp32"] = round(timed(run, a.steps, a.warmup), 3)
    print(json.dumps({"decoder_alone_ms": alone, "images": 3 * B, "speedup": round(alone["fp32"] / alone["bf16"], 3)}), flush=True)
    t32 = launch_table(srr, ins, False, a.steps)
    t16 = launch_table(srr, ins, True, a.steps)
    print(json.dumps({"decoder_launch_sum_ms": {"fp32": round(t32, 2), "bf16": round(t16, 2)}}))


if __name__ == "__main__":
    main()
