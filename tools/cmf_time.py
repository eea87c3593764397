#!/usr/bin/env python3
"""Timing of the `cmf` architecture: ms per training step (fwd + bwd + Adam, stereo_loss3) at 576x960, batch 4; eval ms per
pair at batch 1; and the super-resolution decoder's share of the training step (the decoder alone, forward + backward, on
inputs of the step's shapes).  Also the new decoder kernels one by one, with their HBM traffic / MFMA work per call.

Usage: python tools/cmf_time.py [--steps N] [--warmup W] [--kernels]  -> one JSON line (and a table with --kernels)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ecm_amd  # noqa: E402
from oracle.weights import tensor_for  # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s, MI355X
MFMA_FP32_PEAK = 157.3e12    # flop/s, v_mfma_f32_32x32x2_f32 over 256 CUs


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    ops = ecm_amd.ops
    dev = torch.device("cuda")
    model = ecm_amd.get_model("cmf")
    model.load_state_dict({k: tensor_for(k, v.shape) for k, v in model.state_dict().items()})
    model = model.to(dev).train()
    B, H, W = 4, 576, 960
    g = torch.Generator(device="cpu").manual_seed(1234)
    left, right = torch.randn(B, 3, H, W, generator=g).to(dev), torch.randn(B, 3, H, W, generator=g).to(dev)
    gt = (torch.rand(B, H, W, generator=g) * 191.0).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), fused=True)

    def step():
        opt.zero_grad(set_to_none=True)
        loss, _ = ops.stereo_loss3(model(left, right), gt, 192)
        loss.backward()
        opt.step()

    step_ms = timed(step, a.steps, a.warmup)
    srr = model.srr
    h, w = H // 4, W // 4
    preds = (torch.rand(3, B, h, w, generator=g) * 47.0).to(dev).requires_grad_()
    ref = torch.randn(B, 32, h, w, generator=g).to(dev).requires_grad_()
    half = torch.randn(B, 32, 2 * h, 2 * w, generator=g).to(dev).requires_grad_()
    gy = torch.randn(3, B, 1, H, W, generator=g).to(dev)

    def dec():
        srr.zero_grad(set_to_none=True)
        out = srr(preds, left, ref, half)
        torch.autograd.backward(out, gy)

    def dec_fwd():
        with torch.no_grad():
            srr(preds, left, ref, half)

    dec_ms = timed(dec, a.steps, a.warmup)
    dec_fwd_ms = timed(dec_fwd, a.steps, a.warmup)
    model.eval()
    l1, r1 = left[:1].contiguous(), right[:1].contiguous()

    def ev():
        with torch.no_grad():
            model(l1, r1)

    eval_ms = timed(ev, a.steps, a.warmup)
    out = {"arch": "cmf", "train_576x960_b4_ms_per_step": round(step_ms, 2), "train_pairs_per_s": round(B * 1000 / step_ms, 2),
           "eval_576x960_b1_ms_per_pair": round(eval_ms, 2), "decoder_fwd_bwd_ms": round(dec_ms, 2),
           "decoder_fwd_ms": round(dec_fwd_ms, 2), "decoder_share_of_step": round(dec_ms / step_ms, 3)}
    print(json.dumps(out), flush=True)
    if not a.kernels:
        return
    # ---- the new kernels alone, at the decoder's shapes (3B = 12 images: the three heads as one batch)
    NB = 3 * B
    x96 = torch.randn(NB, 96, H, W, device=dev)
    w1 = torch.randn(1, 96, 3, 3, device=dev) * 0.05
    b1 = torch.zeros(1, device=dev)
    y1 = ops.conv2d_c1_relu(x96, w1, b1)
    g1 = torch.randn_like(y1)
    nb = ecm_amd._lib.query("ecm_conv2d_c1_wgrad_scratch_bytes", NB, 96, H, W)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    gx = torch.empty_like(x96)
    gw, gb = torch.empty_like(w1), torch.empty(1, device=dev)
    P, S = ops._p, ops._stream
    import ctypes
    rows = []
    plane = NB * H * W * 4
    t = timed(lambda: ecm_amd._lib.call("ecm_conv2d_c1_fwd", P(x96), P(w1), P(b1), P(y1), NB, 96, H, W, S()), a.steps, a.warmup)
    rows.append(("conv_out fwd (96->1, relu)", t, 97 * plane, 0))
    t = timed(lambda: ecm_amd._lib.call("ecm_conv2d_c1_dgrad", P(g1), P(y1), P(w1), P(gx), NB, 96, H, W, S()), a.steps, a.warmup)
    rows.append(("conv_out dgrad (1->96)", t, 98 * plane, 0))
    t = timed(lambda: ecm_amd._lib.call("ecm_conv2d_c1_wgrad", P(x96), P(g1), P(y1), P(gw), P(gb), P(scratch),
                                        ctypes.c_longlong(nb), NB, 96, H, W, S()), a.steps, a.warmup)
    rows.append(("conv_out wgrad + bias grad", t, 98 * plane, 0))
    del x96, gx
    for hh, ww in ((h, w), (2 * h, 2 * w)):
        xi = torch.randn(NB, 96, hh, ww, device=dev)
        wd = torch.randn(96, 64, 3, 3, device=dev) * 0.05
        bd = torch.zeros(64, device=dev)
        yd = ops.deconv2d_k3s2_bias(xi, wd, bd)
        gyd = torch.randn_like(yd)
        t = timed(lambda: ops.deconv2d_k3s2_bias(xi, wd, bd), a.steps, a.warmup)
        flop = 2.0 * NB * 96 * 64 * 9 * hh * ww
        rows.append((f"deconv 96->64 fwd+bias {hh}x{ww}->{2 * hh}x{2 * ww}", t, 0, flop))
        pk = ops._pack2d(wd, False)
        t = timed(lambda: ops._conv2d_run(gyd, pk, 96, 3, 3, 2, 1, 1, 1, hh, ww), a.steps, a.warmup)
        rows.append((f"deconv dgrad = conv s2 64->96 COT-3 {2 * hh}x{2 * ww}", t, 0, flop))
        t = timed(lambda: ops.channel_sum(gyd), a.steps, a.warmup)
        rows.append((f"deconv bias grad (channel_sum) {2 * hh}x{2 * ww}", t, gyd.numel() * 4, 0))
        del xi, yd, gyd
    print(f"{'kernel':58s} {'ms':>8s} {'TB/s':>7s} {'of 8 TB/s':>9s} {'TFLOP/s':>8s} {'of fp32 MFMA':>12s}")
    for name, ms, nbytes, flop in rows:
        bw = nbytes / (ms * 1e-3) if nbytes else 0.0
        fl = flop / (ms * 1e-3) if flop else 0.0
        print(f"{name:58s} {ms:8.3f} {bw / 1e12:7.2f} {bw / HBM_PEAK:9.1%} {fl / 1e12:8.1f} {fl / MFMA_FP32_PEAK:12.1%}")


if __name__ == "__main__":
    main()
