#!/usr/bin/env python3
"""What the KITTI training transform costs in the frame decode, at 256 x 512 windows of 375 x 1242 packed
frames, B = 4 and B = 16.  Per case, device events around each call on preallocated operands, the sides alternating inside one
loop, medians with the lowest and the highest sample beside them:
  * ecma_frame_prep_jitter_fwd with all four operations in every view (the reduction launch and the apply launch);
  * the same entry with brightness, saturation and hue but no contrast (the apply launch alone: no reduction is launched);
    the difference of the two is the reduction launch plus one blend per pixel, and is reported as such, not as a measurement
    of the reduction kernel;
  * the entry with no operation at all (the decode's own cost in this kernel);
  * ops.frame_prep_jitter and ops.frame_prep on the same windows, with their checks and host arrays;
  * ecm_frame_prep_packed on the same windows (the path jitter=None takes).
Then the feeder's sustained pairs per second over a shard of such frames with and without `jitter`, the consumer doing nothing
but waiting for each batch, and, where Pillow imports, the host time of the same jitter on one 256 x 512 view with Pillow.
Usage: python tools/jitter_time.py [--iters 200] [--out profiles/r33_jitter_time.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecm_amd  # noqa: E402

H, W, TH, TW = 375, 1242, 256, 512


def samples(fns, iters, warmup):
    """[median, lowest, highest] time in ms of each callable between two device events, alternating them."""
    times = [[] for _ in fns]
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            e.synchronize()
            if i >= warmup:
                times[j].append(s.elapsed_time(e))
    return [[round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_jitter_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib = ecm_amd.ops, ecm_amd._lib
    shards = importlib.import_module(ops.__name__.rsplit(".", 1)[0] + ".shards")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                              # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                               # noqa: E731
    host = lambda t, v: C.cast((t * len(v))(*v), C.c_void_p)                                       # noqa: E731
    g = torch.Generator().manual_seed(0)
    rows = []
    for B in (4, 16):
        rgb = torch.randint(0, 256, (B, H, W, 6), dtype=torch.uint8, generator=g).cuda()
        dsp = (torch.rand(B, H, W, generator=g) * 200).half().cuda()
        rng = random.Random(B)
        ys, xs = [rng.randint(0, H - TH) for _ in range(B)], [rng.randint(0, W - TW) for _ in range(B)]
        left, right, image = (torch.empty(B, 3, TH, TW, device="cuda") for _ in range(3))
        disp = torch.empty(B, TH, TW, device="cuda")
        nbytes = lib.query("ecma_jitter_scratch_bytes", 2 * B, TH, TW)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        params = {"four operations": ops.jitter_params(B, random.Random(1), torch.Generator().manual_seed(2)),
                  "no contrast": ops.jitter_params(B, random.Random(1), torch.Generator().manual_seed(2), contrast=0),
                  "no operation": ops.jitter_params(B, random.Random(1), torch.Generator().manual_seed(2), brightness=0, contrast=0,
                                                    saturation=0, hue=0)}
        mean, std = host(C.c_float, ops.FLYING3D_MEAN), host(C.c_float, ops.FLYING3D_STD)
        yh, xh = host(C.c_int, ys), host(C.c_int, xs)

        def entry(q):
            f, o, h, pc = (host(C.c_float, q.factors.reshape(-1).tolist()), host(C.c_int, q.order.reshape(-1).tolist()),
                           host(C.c_int, q.hue_shift.reshape(-1).tolist()), host(C.c_float, q.pca.reshape(-1).tolist()))
            return lambda: lib.call("ecma_frame_prep_jitter_fwd", p(rgb), p(dsp), 1, p(left), p(right), p(disp), p(image), B, H, W, yh, xh, TH, TW,
                                    f, o, h, pc, mean, std, p(scratch), C.c_longlong(nbytes), st())
        fns = [entry(q) for q in params.values()] + [
            lambda: lib.call("ecm_frame_prep_packed", p(rgb), p(dsp), 1, p(left), p(right), p(disp), p(image), B, H, W, yh, xh, TH, TW, TH, 0,
                             mean, std, 0, st()),
            lambda: ops.frame_prep_jitter((rgb, dsp), ys, xs, TH, TW, params["four operations"], want_image=True),
            lambda: ops.frame_prep((rgb, dsp), ys, xs, TH, TW, want_image=True)]
        four, three, none, prep, op, op_prep = samples(fns, a.iters, a.warmup)
        px = B * TH * TW
        row = {"B": B, "window": [TH, TW], "frame": [H, W], "entry_four_operations_ms": four, "entry_without_contrast_ms": three,
               "entry_no_operation_ms": none, "ecm_frame_prep_packed_ms": prep, "ops_frame_prep_jitter_ms": op, "ops_frame_prep_ms": op_prep,
               "reduction_launch_plus_one_blend_ms": round(four[0] - three[0], 4), "four_operations_over_frame_prep": round(four[0] / prep[0], 2),
               "bytes_read": px * 8 * 2, "bytes_written": px * 40,
               "GB_per_s_four_operations": round((px * 8 * 2 + px * 40) / four[0] / 1e6, 1), "GB_per_s_frame_prep": round(px * 48 / prep[0] / 1e6, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the feeder
    rs = np.random.RandomState(0)
    with tempfile.TemporaryDirectory() as tmp:
        frames = [np.concatenate([rs.randint(0, 256, (H, W, 6)).astype(np.float32), rs.rand(H, W, 1).astype(np.float32) * 200], 2)
                  for _ in range(a.frames)]
        reader = shards.ShardReader(shards.write_shard(frames, os.path.join(tmp, "s.ecms"), "fp16"))
        del frames
        for B in (4, 16):
            row = {"feeder": True, "B": B, "frames": a.frames, "epochs": a.epochs}
            for name, jitter in (("jitter=None", None), ("jitter=KITTI_JITTER", dict(ops.KITTI_JITTER))):
                f = shards.ShardFeeder(reader, batch=B, split="train", seed=1, kitti=True, jitter=jitter)
                rates = []
                for epoch in range(a.epochs + 1):                           # the first epoch warms the pinned buffers up
                    torch.cuda.synchronize()
                    t0, n = time.perf_counter(), 0
                    for batch in f:
                        n += B
                    torch.cuda.synchronize()
                    if epoch:
                        rates.append(n / (time.perf_counter() - t0))
                f.close()
                row[name + " pairs_per_s"] = [round(statistics.median(rates), 1), round(min(rates), 1), round(max(rates), 1)]
            rows.append(row)
            print(json.dumps(row), flush=True)
    pillow = None
    try:
        import PIL
        from PIL import Image, ImageEnhance
        img = Image.fromarray(rs.randint(0, 256, (TH, TW, 3)).astype(np.uint8), "RGB")
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            im = ImageEnhance.Brightness(img).enhance(0.83)
            im = ImageEnhance.Contrast(im).enhance(1.17)
            im = ImageEnhance.Color(im).enhance(1.4)
            h, s, v = im.convert("HSV").split()
            nh = np.array(h, dtype=np.uint8)
            nh += np.uint8(77)
            Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
            ts.append((time.perf_counter() - t0) * 1e3)
        pillow = {"version": PIL.__version__, "host_ms_per_view": [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]}
    except ImportError:
        pass
    res = {"what": "entries alone on preallocated operands, ops with their checks and host arrays; each entry [median, lowest, highest] in ms; "
                   "the feeder in pairs per second per epoch, the consumer only waiting",
           "iters": a.iters, "timing": "device events around each call, alternating inside one loop", "device": torch.cuda.get_device_name(0),
           "rows": rows, "pillow": pillow if pillow else "Pillow does not import on this machine: no host-side time"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
