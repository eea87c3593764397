#!/usr/bin/env python3
"""The split-bf16 kernels (ops.split_products, csrc/split_bf16.hip) against the fp32 kernels they stand in for, in ONE process.

Per-launch times of the four stride-2 layers of the hourglass at batch 4 of the bench geometry (576x960, 1/4-resolution volume
48x144x240), forward and data gradient each: the split kernel and the fp32 kernel run in alternating rounds on the same random
operands, weights packed beforehand; median and minimum over the rounds.  Rates are direct-form FLOPs (2 * 27 * Ci * Co per output
voxel of the convolution / input voxel of the transposed convolution) against the fp32 MFMA peak and against the register-only
bf16x3 ceiling of profiles/r04_bf16x3_micro.txt.  Then the cmfsm training step at 4x576x960 with all four kinds on and with the switch off,
alternating.

Usage: python tools/split_bf16_time.py [--rounds N] [--reps R] [--steps K] [--out profiles/r10_split_bf16_time.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ecm_amd  # noqa: E402
from oracle.weights import tensor_for  # noqa: E402

ops = ecm_amd.ops
MFMA_F32_PEAK = 157.3e12        # flop/s dense, v_mfma_f32_32x32x2_f32
BF16X3_CEILING = 413e12         # fp32-equivalent flop/s, six bf16 MFMAs per product from registers (profiles/r04_bf16x3_micro.txt)
# (layer, kind, kernel Ci -> Co, the volume the kernel reads [D,H,W], the volume it writes)
LAYERS = [
    ("conv 32->64 @ (48,144,240)", "conv", 32, 64, (48, 144, 240)),
    ("conv 64->64 @ (24,72,120)", "conv", 64, 64, (24, 72, 120)),
    ("deconv 64->64 from (12,36,60)", "deconv", 64, 64, (12, 36, 60)),
    ("deconv 64->32 from (24,72,120)", "deconv", 64, 32, (24, 72, 120)),
]


def ms_of(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def ab(fa, fb, rounds, reps):
    """fa and fb in alternating rounds; (median, min) of each in ms."""
    for _ in range(2):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(ms_of(fa, reps))
        tb.append(ms_of(fb, reps))
    return (statistics.median(ta), min(ta)), (statistics.median(tb), min(tb))


def layer_rows(B, rounds, reps):
    g = torch.Generator(device="cpu").manual_seed(1234)
    rows = []
    for label, op, Ci, Co, dims in LAYERS:
        up = tuple(2 * d for d in dims)
        small = tuple((d - 1) // 2 + 1 for d in dims)
        if op == "conv":
            w = (torch.randn(Co, Ci, 3, 3, 3, generator=g) * (2.0 / (27 * Ci)) ** 0.5).cuda()
            x, gy = torch.randn(B, Ci, *dims, generator=g).cuda(), torch.randn(B, Co, *small, generator=g).cuda()
            vox = small[0] * small[1] * small[2]
            pk32, pks = ops._pack_conv(w), ops._pack_split(w, False)
            dk32, dks = ops._pack_deconv(w), ops._pack_split(w, True)
            runs = [("conv_fwd", lambda: ops._split_conv_fwd(x, pks, Co), lambda: ops._conv_fwd(x, pk32, Co, 2)),
                    ("conv_dgrad", lambda: ops._split_deconv_fwd(gy, dks, Ci, dims), lambda: ops._deconv_fwd(gy, dk32, Ci, dims))]
        else:
            w = (torch.randn(Ci, Co, 3, 3, 3, generator=g) * (2.0 / (27 * Ci)) ** 0.5).cuda()
            x, gy = torch.randn(B, Ci, *dims, generator=g).cuda(), torch.randn(B, Co, *up, generator=g).cuda()
            vox = dims[0] * dims[1] * dims[2]
            pk32, pks = ops._pack_deconv(w), ops._pack_split(w, True)
            dk32, dks = ops._pack_conv(w), ops._pack_split(w, False)
            runs = [("deconv_fwd", lambda: ops._split_deconv_fwd(x, pks, Co, up), lambda: ops._deconv_fwd(x, pk32, Co, up)),
                    ("deconv_dgrad", lambda: ops._split_conv_fwd(gy, dks, Ci), lambda: ops._conv_fwd(gy, dk32, Ci, 2))]
        flop = 2.0 * 27 * Ci * Co * vox * B
        for kind, fs, f32 in runs:
            (ms, mns), (m32, mn32) = ab(fs, f32, rounds, reps)
            rows.append({"layer": label, "kind": kind, "B": B, "split_ms_median": round(ms, 4), "split_ms_min": round(mns, 4),
                         "fp32_ms_median": round(m32, 4), "fp32_ms_min": round(mn32, 4), "speedup_median": round(m32 / ms, 3),
                         "split_tflops": round(flop / ms / 1e9, 1), "fp32_tflops": round(flop / m32 / 1e9, 1),
                         "fp32_of_mfma_peak": round(flop / m32 / 1e-3 / MFMA_F32_PEAK, 3),
                         "split_of_bf16x3_ceiling": round(flop / ms / 1e-3 / BF16X3_CEILING, 3)})
            print(json.dumps(rows[-1]), flush=True)
            del fs, f32
        del x, gy, w, runs
        torch.cuda.empty_cache()
    return rows


def step_row(B, H, W, rounds, steps):
    model = ecm_amd.get_model("cmfsm")
    model.load_state_dict({k: tensor_for(k, v.shape) for k, v in model.state_dict().items()})
    model = model.cuda().train()
    g = torch.Generator(device="cpu").manual_seed(99)
    left, right = torch.randn(B, 3, H, W, generator=g).cuda(), torch.randn(B, 3, H, W, generator=g).cuda()
    gt = (torch.rand(B, H, W, generator=g) * 191.0).cuda()

    def step(mode):
        def run():
            for p in model.parameters():
                p.grad = None
            with ops.split_products(mode, ops.SPLIT_ALL_KINDS):
                loss, _ = ops.stereo_loss3(model(left, right), gt, 192)
                loss.backward()
                ops.join_side_streams()
        return run
    (on, on_min), (off, off_min) = ab(step("bf16x3"), step("fp32"), rounds, steps)
    row = {"step": "cmfsm train fwd+loss+bwd", "B": B, "hw": [H, W], "kinds": sorted(ops.SPLIT_ALL_KINDS),
           "split_ms_median": round(on, 2), "split_ms_min": round(on_min, 2), "fp32_ms_median": round(off, 2),
           "fp32_ms_min": round(off_min, 2), "speedup_median": round(off / on, 4)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "method": "alternating rounds in one process; median and min over rounds",
           "layers": layer_rows(a.batch, a.rounds, a.reps)}
    if not a.no_step:
        out["step"] = step_row(a.batch, 576, 960, max(3, a.rounds // 2), a.steps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
