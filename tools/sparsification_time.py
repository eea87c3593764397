#!/usr/bin/env python3
"""What the sparsification curves cost, B = 4 at 576 x 960 and at 384 x 1248, K = 3 measures, 20 steps:
ops.eval_sparsification (nine launches of csrc/eval_sparsify.hip, its allocations and the torch ops that form the areas), the
entry point alone on preallocated outputs, and the torch.sort-based restatement of tests/test_sparsification_cpu.py (curve_t: a
stable sort of the 64-bit keys, cumulative sums and two searches per plane and sample) on the same device tensors -- the only
baseline there is.  Each sample is the device-event time over `burst` back-to-back calls, divided by `burst`; the sides alternate
inside one loop.  Bytes: the four streaming passes read pred, gt and the K planes once each; the share is of the 6 TB/s streaming
ceiling of DESIGN.md section 3.
Usage: python tools/sparsification_time.py [--iters 30] [--burst 10] [--out profiles/r18_sparsification_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ecm_amd  # noqa: E402

FRAMES = ((576, 960), (384, 1248))
CEILING = 6.0e12


def samples(fns, bursts, iters, warmup):
    """[median, lowest, highest] device time in ms per call of each callable, alternating them."""
    times = [[] for _ in fns]
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(bursts[j]):
                fn()
            e.record()
            e.synchronize()
            if i >= warmup:
                times[j].append(s.elapsed_time(e) / bursts[j])
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_sparsification_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from test_sparsification_cpu import curve_t, kernel_constants, measure_key, pixel_terms, sparsify_t
    ops, lib = ecm_amd.ops, ecm_amd._lib
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    B, K, steps, levels = 4, 3, 20, kernel_constants()["LEVELS"]
    rows = []
    for H, W in FRAMES:
        gt = torch.rand(B, H, W, device="cuda", generator=g) * 200.0 - 4.0                       # ~4 % outside (0, 192)
        noise = torch.randn(B, H, W, device="cuda", generator=g)
        pred = gt + noise * 1.5 * (1 + 4 * (torch.rand(B, H, W, device="cuda", generator=g) < 0.1))
        e = (pred - gt).abs()
        # stand-ins for std, entropy and -peak: one follows the error loosely, one is pure noise, one saturates (a third of the
        # pixels share the value -1.0: a tie group)
        ms = [e * torch.rand_like(e) + 0.3, torch.rand(B, H, W, device="cuda", generator=g) * 5,
              -torch.clamp(torch.rand(B, H, W, device="cuda", generator=g) * 1.5, max=1.0)]
        table = torch.empty(B, K + 1, steps, 2, device="cuda")
        count = torch.empty(B, 3, device="cuda", dtype=torch.int64)
        need = lib.query("ecm_eval_sparsify_scratch_bytes", B, H, W, K, steps)
        scratch = torch.empty(need, device="cuda", dtype=torch.uint8)
        ptrs = (C.c_void_p * K)(*(m.data_ptr() for m in ms))

        def restatement():
            out = []
            for b in range(B):
                mask, E, bad = pixel_terms(pred[b].reshape(-1), gt[b].reshape(-1), 192)
                out += [curve_t(measure_key(m[b].reshape(-1)[mask]), E, bad, steps) for m in ms] + [curve_t(E, E, bad, steps)]
            return torch.stack(out)

        fns = (lambda: lib.call("ecm_eval_sparsify", p(pred), p(gt), ptrs, p(table), p(count), p(scratch), C.c_longlong(need),
                                B, H, W, K, steps, C.c_float(192.0), st()),
               lambda: ops.eval_sparsification(pred, gt, ms, 192, steps),
               restatement)
        entry, op, torch_ms = samples(fns, (a.burst, a.burst, 1), a.iters, a.warmup)
        want_table, want_count = sparsify_t(pred.cpu(), gt.cpu(), [m.cpu() for m in ms], 192, steps)
        sp = ops.eval_sparsification(pred, gt, ms, 192, steps)
        got = torch.cat([torch.stack([sp.epe, sp.d1], -1), torch.stack([sp.oracle_epe, sp.oracle_d1], -1).unsqueeze(1)], 1).cpu()
        ulp = int((got.view(torch.int32).long() - want_table.view(torch.int32).long()).abs().max())
        nbytes = levels * (K + 2) * 4 * B * H * W
        row = {"frame": [H, W], "B": B, "K": K, "steps": steps, "entry_ms": entry, "op_ms": op, "torch_sort_ms": torch_ms,
               "torch_over_op": round(torch_ms[0] / op[0], 2), "streamed_bytes": nbytes,
               "entry_tb_per_s": round(nbytes / (entry[0] * 1e-3) / 1e12, 3),
               "share_of_streaming_ceiling": round(nbytes / (entry[0] * 1e-3) / CEILING, 3), "scratch_bytes": int(need),
               "count_identical_to_sparsify_t": bool(torch.equal(sp.count.cpu(), want_count)), "table_ulp_from_sparsify_t": ulp,
               "valid_share": round(float(sp.count[:, 0].sum()) / (B * H * W), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"what": "ecm_eval_sparsify on preallocated outputs (entry), ops.eval_sparsification with its allocations and the area "
                   "ops (op), and the torch.sort-based restatement on the same device tensors (torch_sort); each entry "
                   "[median, lowest, highest] in ms per call",
           "kernel_constants": kernel_constants(), "iters": a.iters, "burst": a.burst,
           "timing": "device events over `burst` back-to-back calls (the restatement: one call), alternating inside one loop",
           "ceiling_bytes_per_s": CEILING, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
