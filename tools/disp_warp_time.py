#!/usr/bin/env python3
"""What the temporal carry costs, at 576 x 960 and 384 x 1248, B = 1 and 4, on a ramp-and-step scene warped
by a forward motion that magnifies by about 1.05, under both footprints, with three attribute planes (what DisparityTracker
carries).  Per case: the warp's launch set alone on preallocated outputs (ecmt_disparity_warp_fwd: the memset of the keys, the
scatter, the resolve), ops.disparity_warp with its allocations, the same result computed by ATen on the same tensors -- an fp64
matmul with M, the divisions, int64 keys through scatter_reduce_("amax"), the attributes by gather -- the fusion launch, and a plain
device copy, whose rate stands for the streaming ceiling.  Bytes the warp must move per pixel: 4 (disp) + 8 (the memset) + 8 (at
least one atomic) + 8 (the keys read back) + 4 + 4 (out, src) + 8 C (attributes gathered and stored): 36 + 8 C; the further
atomics of "cover" (up to three more per pixel) are left out of the denominator, so its share is on the low side.
Then DisparityTracker per frame against model.predict alone (cmfsm, B = 1, 576 x 960).
Device events around each call, medians with the lowest and the highest sample beside them; the sides alternate inside one loop.
Usage: python tools/disp_warp_time.py [--iters 200] [--out profiles/r26_disp_warp_time.json]"""
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

FRAMES = ((576, 960), (384, 1248))
ATTRS = 3


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


def scene(B, H, W):
    """A ramp (the ground: disparity growing down the image) with a step (a box in front of it)."""
    y = torch.arange(H, device="cuda", dtype=torch.float32).view(1, H, 1)
    d = (4.0 + 60.0 * y / H).expand(B, H, W).clone()
    d[:, H // 3:2 * H // 3, W // 3:W // 2] = 90.0
    return d.contiguous()


def aten_warp(d, M, attrs, nearest):
    """The ATen restatement on the device (the rule of tests/test_disp_warp_cpu.py::warp_t, with the matrix product as a matmul)."""
    B, H, W = d.shape
    dev = d.device
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    v = torch.stack([x.expand(B, H, W), y.expand(B, H, W), d.double(), torch.ones(B, H, W, device=dev, dtype=torch.float64)], 1)
    r = torch.matmul(M.view(1, 4, 4), v.view(B, 4, H * W)).view(B, 4, H, W)
    w = r[:, 3]
    u, vv, dn = r[:, 0] / w, r[:, 1] / w, (r[:, 2] / w).float()
    cand = torch.isfinite(d) & (d > 0) & torch.isfinite(w) & (w != 0) & torch.isfinite(dn) & (dn > 0) \
        & (u >= 0) & (u <= W - 1) & (vv >= 0) & (vv <= H - 1)
    key = dn.view(torch.int32).long() * (1 << 32) + torch.arange(H * W, device=dev).view(1, H, W)
    zero = torch.zeros_like(key)
    u, vv = torch.where(cand, u, 0.0), torch.where(cand, vv, 0.0)
    best = torch.zeros(B, H * W, dtype=torch.int64, device=dev)

    def land(yy, xx, on):
        best.scatter_reduce_(1, (yy * W + xx).view(B, -1), torch.where(on, key, zero).view(B, -1), "amax")

    if nearest:
        land((vv + 0.5).floor().long().clamp(max=H - 1), (u + 0.5).floor().long().clamp(max=W - 1), cand)
    else:
        fu, fv = u.floor(), vv.floor()
        x0, y0, right, down = fu.long(), fv.long(), cand & (u > fu), cand & (vv > fv)
        x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
        land(y0, x0, cand)
        land(y0, x1, right)
        land(y1, x0, down)
        land(y1, x1, right & down)
    hole = best == 0
    out = torch.where(hole, 0.0, (best >> 32).to(torch.int32).view(torch.float32))
    src = torch.where(hole, -1, best & 0xFFFFFFFF)
    got = attrs.flatten(2).gather(2, src.clamp(min=0).unsqueeze(1).expand(-1, attrs.shape[1], -1))
    return out.view(B, 1, H, W), src.view(B, 1, H, W), torch.where(hole.unsqueeze(1), 0.0, got).view(attrs.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tracker-iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_disp_warp_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib, models = ecm_amd.ops, ecm_amd._lib, ecm_amd.models
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                            # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for H, W in FRAMES:
        Q = ops.q_matrix(721.5, 0.54, 0.5 * W + 0.37, 0.5 * H + 0.21)
        T = torch.eye(4, dtype=torch.float64)
        T[2, 3] = -0.05 * 721.5 * 0.54 / 34.0                              # Z = f b / d: the mid-scene depth (d = 34) shrinks by 1/1.05
        M = ops.warp_matrix(Q, T).cuda()
        for B in (1, 4):
            n = B * H * W
            d = scene(B, H, W)
            attrs = torch.rand(B, ATTRS, H, W, device="cuda", generator=g)
            var = 0.05 + torch.rand(B, 1, H, W, device="cuda", generator=g)
            a_buf = torch.randn(8 * n, device="cuda", generator=g)        # 32 B per pixel in, 32 out: one copy moves 64 B per pixel
            b_buf = torch.empty_like(a_buf)
            out, src = torch.empty(B, 1, H, W, device="cuda"), torch.empty(B, 1, H, W, device="cuda", dtype=torch.int32)
            attrs_out = torch.empty_like(attrs)
            nb = lib.query("ecmt_disparity_warp_scratch_bytes", B, H, W)
            scratch = torch.empty(nb, device="cuda", dtype=torch.uint8)
            for fp, footprint in enumerate(ops.WARP_FOOTPRINTS):
                warped, carried, _ = ops.disparity_warp(d, M, None, attrs, footprint=footprint, with_source=True)
                fns = (lambda: lib.call("ecmt_disparity_warp_fwd", p(d), None, p(M), 0, p(attrs), ATTRS, p(out), p(src), p(attrs_out),
                                        p(scratch), C.c_longlong(nb), B, H, W, 0.0, 3e38, fp, st()),
                       lambda: ops.disparity_warp(d, M, None, attrs, footprint=footprint, with_source=True),
                       lambda: aten_warp(d, M, attrs, fp == 1),
                       lambda: ops.disparity_fuse(d, var, warped, carried[:, 0:1], None, carried[:, 1:2], 3.0, 0.01, True),
                       lambda: b_buf.copy_(a_buf))
                launches, op, aten, fuse, copy = samples(fns, a.iters, a.warmup)
                got, want = ops.disparity_warp(d, M, None, attrs, footprint=footprint, with_source=True), aten_warp(d, M, attrs, fp == 1)
                same = torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[2].long(), want[1]) \
                    and torch.equal(got[1].view(torch.int32), want[2].view(torch.int32))
                ceiling = 2 * a_buf.numel() * 4 / (copy[0] * 1e-3)                       # bytes per second of the copy
                nbytes = n * (36 + 8 * ATTRS)
                row = {"frame": [H, W], "B": B, "footprint": footprint, "attributes": ATTRS, "holes": round(float((got[2] < 0).sum()) / n, 4),
                       "warp_launches_ms": launches, "warp_ms": op, "aten_warp_ms": aten, "fuse_ms": fuse, "copy_ms": copy,
                       "copy_GBps": round(ceiling / 1e9, 1), "warp_bytes_per_pixel": 36 + 8 * ATTRS,
                       "warp_share_of_ceiling": round(nbytes / ceiling / (launches[0] * 1e-3), 4),
                       "aten_over_warp": round(aten[0] / op[0], 2), "equal_to_aten_bit_for_bit": same}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del a_buf, b_buf
            torch.cuda.empty_cache()
    # the tracker per frame against predict alone
    H, W = FRAMES[0]
    torch.manual_seed(5)
    model = ecm_amd.get_model("cmfsm").cuda().eval()
    left, right = (torch.randn(1, 3, H, W, device="cuda", generator=g) for _ in range(2))
    Q = ops.q_matrix(721.5, 0.54, 0.5 * W, 0.5 * H)
    T = torch.eye(4, dtype=torch.float64)
    T[2, 3] = -0.5
    tracker = models.DisparityTracker(model, Q)
    tracker(left, right)
    predict, tracked = samples((lambda: model.predict(left, right, (2,)), lambda: tracker(left, right, motion=T)), a.tracker_iters, 5)
    frame = {"arch": "cmfsm", "frame": [H, W], "B": 1, "predict_ms": predict, "tracker_ms": tracked,
             "tracker_minus_predict_ms": round(tracked[0] - predict[0], 4), "iters": a.tracker_iters}
    print(json.dumps(frame), flush=True)
    res = {"what": "the warp's launch set alone on preallocated outputs (memset, scatter, resolve; 3 attribute planes), ops.disparity_warp "
                   "with its allocations, the same result by ATen on the same tensors (fp64 matmul, int64 scatter_reduce amax, gather), "
                   "the fusion launch with its allocations and a device copy of 32 B per pixel; each entry [median, lowest, highest] in "
                   "ms.  warp_share_of_ceiling = (36 + 8 C bytes per pixel) / (the copy's bytes per second) / (the median time of the "
                   "launch set).  tracker: DisparityTracker per frame against model.predict alone",
           "iters": a.iters, "timing": "device events around each call, alternating inside one loop", "rows": rows, "tracker": frame}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
