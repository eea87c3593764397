#!/usr/bin/env python3
"""ops.eval_kitti against the reference's torch statements (eval_kitti.py:84-103 with its three `.item()` calls) for one KITTI
validation batch on the device.  Prints one JSON line.  Usage: python tools/eval_kitti_time.py [--batch 4] [--iters 200]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ecm_amd  # noqa: E402

STREAM_CEILING = 6.0e12          # bytes/s: DESIGN.md section 3, ATen `add` on this part


def torch_statements(output3, disparity, ones, zeros):
    local = torch.arange(disparity.shape[-1], device=disparity.device).float().expand_as(disparity)
    mask = (disparity < 192) & (disparity > 0)
    mask_non = mask & ((local - disparity) >= 0)
    o = torch.squeeze(output3, 1)
    loss = torch.mean(torch.abs(o[mask] - disparity[mask]))
    loss_non = torch.mean(torch.abs(o[mask_non] - disparity[mask_non]))
    torch.mean(torch.abs(o[mask_non] - disparity[mask_non]))                     # loss_true: computed, never read
    e = torch.abs(o[mask] - disparity[mask])
    good = torch.where((e < 3) | (e < 0.05 * disparity[mask]), ones, zeros)
    total = torch.where(disparity[mask] > 0, ones, zeros)
    loss_3 = 100 - torch.sum(good) / torch.sum(total) * 100
    return loss.item(), loss_non.item(), loss_3.item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    B, H, W = a.batch, 384, 1248
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(B, H, W, generator=g) * 200.0
    gt[torch.rand(B, H, W, generator=g) < 0.7] = 0.0                             # KITTI ground truth is sparse
    gt[:, :9], gt[:, :, :6] = 0.0, 0.0
    pred = (gt + torch.randn(B, H, W, generator=g) * 2.0).unsqueeze(1).cuda()
    gt = gt.cuda()
    ones, zeros = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    log = torch.empty(a.iters + a.warmup, 8, device="cuda")

    def hip(i):
        ecm_amd.ops.eval_kitti(pred, gt, out=log[i])

    for i in range(a.warmup):
        hip(i)
        ref = torch_statements(pred, gt, ones, zeros)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.iters):
        hip(a.warmup + i)
    torch.cuda.synchronize()
    hip_host = (time.perf_counter() - t0) / a.iters
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(a.iters):
        hip(a.warmup + i)
    e.record()
    torch.cuda.synchronize()
    hip_dev = s.elapsed_time(e) * 1e-3 / a.iters
    t0 = time.perf_counter()
    for _ in range(a.iters):
        torch_statements(pred, gt, ones, zeros)
    torch.cuda.synchronize()
    ref_host = (time.perf_counter() - t0) / a.iters
    got = log[-1].cpu()
    nbytes = 2 * B * H * W * 4
    print(json.dumps({
        "what": "ops.eval_kitti vs the reference's torch statements (three .item() syncs), one batch", "shape": [B, H, W],
        "bytes_read": nbytes, "iters": a.iters,
        "hip_us_per_call_host_clock": round(hip_host * 1e6, 2), "hip_us_per_call_device_events": round(hip_dev * 1e6, 2),
        "torch_statements_us_per_batch_host_clock": round(ref_host * 1e6, 2),
        "hip_bytes_per_s": round(nbytes / hip_dev, 0), "fraction_of_6TBs_stream_ceiling": round(nbytes / hip_dev / STREAM_CEILING, 4),
        "speedup_over_torch_statements": round(ref_host / hip_host, 1),
        "hip": [float(got[0]), float(got[1]), float(got[3])], "torch": list(ref)}))


if __name__ == "__main__":
    main()
