#!/usr/bin/env python3
"""What the dense disparity alignment costs, at 576 x 960, B = 1 and 4, step 1 and 2, on a ramp-and-step
scene seen again after a small motion.  Per case: the launch set of ecmm_align_normal_fwd alone on preallocated buffers (the
accumulating and the finishing launch), ops.motion_normal with its allocations and its one host-to-device copy of the matrices,
the same sums computed by ATen on the same device tensors (an fp64 restatement of include/ecm_motion.h: elementwise planes, a
four-tap gather, [B,N,6] Jacobians, an einsum for J^T J), and a plain device copy whose rate stands for the streaming ceiling.
Bytes the kernel must move per lattice pixel: 4 (disp0) + 4 (weight) + 1 (valid0) + 16 (four taps, mostly cache hits: counted
once as 4) = 13; its arithmetic per used pixel is about 330 fp64 operations and 26 fp64 divisions.
Then ops.motion_estimate per frame (10 iterations allowed), and a StereoOdometry frame against a DisparityTracker frame and
model.predict alone (cmfsm, B = 1, 576 x 960).
Device events around each call, medians with the lowest and the highest sample beside them; the sides alternate inside one loop.
Usage: python tools/motion_align_time.py [--iters 100] [--out profiles/r27_motion_align_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecm_amd  # noqa: E402

H, W = 576, 960
F64 = torch.float64


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


def wall(fn, iters, warmup):
    """[median, lowest, highest] wall time in ms of a callable that synchronises itself (it reads results on the host)."""
    t = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]


def scene(B, shift=0.0):
    """A ramp (the ground: disparity growing down the image) with a step (a box in front of it), moved sideways by `shift` px."""
    y = torch.arange(H, device="cuda", dtype=torch.float32).view(1, H, 1)
    x = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    d = (4.0 + 60.0 * y / H + 0.01 * (x - shift)).expand(B, H, W).clone()
    d[:, H // 3:2 * H // 3, W // 3 + int(shift):W // 2 + int(shift)] = 90.0
    return d.contiguous()


def aten_normal(d0, d1, w, v0, Q, A, T, step, tap_range=1.0, max_residual=3.0, cauchy=1.0):
    """include/ecm_motion.h in ATen on the device (the rule of tests/test_motion_align_cpu.py::align_t, without its book-keeping)."""
    B = d0.shape[0]
    dev = d0.device
    ys, xs = torch.meshgrid(torch.arange(0, H, step, device=dev), torch.arange(0, W, step, device=dev), indexing="ij")
    x, y = xs.to(F64).expand(B, -1, -1), ys.to(F64).expand(B, -1, -1)
    d = d0[:, ::step, ::step]
    ww = w[:, ::step, ::step].to(F64)
    fd = d.to(F64)
    row = lambda m, a, b, c: ((m[0] * a + m[1] * b) + m[2] * c) + m[3]                           # noqa: E731
    P3 = row(Q[3], x, y, fd)
    usable = torch.isfinite(d) & v0[:, ::step, ::step] & (d > 0) & torch.isfinite(P3) & (P3 != 0) & torch.isfinite(ww) & (ww > 0)
    X = [row(Q[i], x, y, fd) / P3 for i in range(3)]
    Y = [row(T[i], X[0], X[1], X[2]) for i in range(3)]
    h = [row(A[q], Y[0], Y[1], Y[2]) for q in range(4)]
    u, v, dn = h[0] / h[3], h[1] / h[3], h[2] / h[3]
    cand = usable & torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(dn) & (dn > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    uc, vc = torch.where(cand, u, 0.0), torch.where(cand, v, 0.0)
    x0, y0 = uc.floor().clamp(max=W - 2).long(), vc.floor().clamp(max=H - 2).long()
    fx, fy = u - x0, v - y0
    flat = d1.reshape(B, -1)
    at = (y0 * W + x0).reshape(B, -1)
    taps = [flat.gather(1, at + o).view_as(u) for o in (0, 1, W, W + 1)]
    ok = lambda t: torch.isfinite(t) & (t > 0)                                                   # noqa: E731
    st = torch.stack(taps)
    used = cand & ok(taps[0]) & ok(taps[1]) & ok(taps[2]) & ok(taps[3]) & ~((st.amax(0) - st.amin(0)).to(F64) > tap_range)
    d00, d01, d10, d11 = (t.to(F64) for t in taps)
    top, bot = d00 + fx * (d01 - d00), d10 + fx * (d11 - d10)
    r = (top + fy * (bot - top)) - dn
    gx = (1.0 - fy) * (d01 - d00) + fy * (d11 - d10)
    gy = (1.0 - fx) * (d10 - d00) + fx * (d11 - d01)
    used = used & (r.abs() <= max_residual)
    J = []
    for j in range(6):
        dh = [A[q, j].expand_as(u) if j < 3 else (A[q, 2] * Y[1] - A[q, 1] * Y[2], A[q, 0] * Y[2] - A[q, 2] * Y[0],
                                                   A[q, 1] * Y[0] - A[q, 0] * Y[1])[j - 3] for q in range(4)]
        du, dv, dd = (dh[0] - u * dh[3]) / h[3], (dh[1] - v * dh[3]) / h[3], (dh[2] - dn * dh[3]) / h[3]
        J.append((gx * du + gy * dv) - dd)
    J = torch.where(used.unsqueeze(-1), torch.stack(J, -1), 0.0).reshape(B, -1, 6)
    r = torch.where(used, r, 0.0).reshape(B, -1)
    a = torch.where(used, ww / (1.0 + ww * r.view_as(ww) * r.view_as(ww) / (cauchy * cauchy)), 0.0).reshape(B, -1)
    Hm = torch.einsum("bn,bni,bnj->bij", a, J, J)
    g = torch.einsum("bn,bni,bn->bi", a, J, r)
    return Hm, g, (a * r * r).sum(1), a.sum(1), used.sum((1, 2)), cand.sum((1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frame-iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_motion_align_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ops, lib, models = ecm_amd.ops, ecm_amd._lib, ecm_amd.models
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None               # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                             # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = ops.q_matrix(721.5, 0.54, 0.5 * W + 0.37, 0.5 * H + 0.21)
    T = ops.se3_exp(torch.tensor([0.02, -0.01, 0.05, 0.002, 0.004, -0.001], dtype=F64))
    mats = torch.cat([Q.reshape(-1), torch.linalg.inv(Q).reshape(-1), T.reshape(-1)]).cuda()
    Qd, Ad, Td = mats[:16].view(4, 4), mats[16:32].view(4, 4), mats[32:].view(4, 4)
    rows = []
    for B in (1, 4):
        d0, d1 = scene(B), scene(B, 2.0)
        w = 0.5 + torch.rand(B, H, W, device="cuda", generator=g)
        v0 = torch.rand(B, H, W, device="cuda", generator=g) > 0.02
        a_buf = torch.randn(8 * B * H * W, device="cuda", generator=g)
        b_buf = torch.empty_like(a_buf)
        sums = torch.empty(B, 32, device="cuda", dtype=F64)
        for step in (1, 2):
            nb = lib.query("ecmm_align_scratch_bytes", B, H, W, step)
            scratch = torch.empty(nb, device="cuda", dtype=torch.uint8)
            v8 = v0.view(torch.uint8)
            fns = (lambda: lib.call("ecmm_align_normal_fwd", p(d0), p(v8), p(w), p(d1), None, p(mats), p(mats, 128), p(mats, 256), 0,
                                    p(sums), None, p(scratch), C.c_longlong(nb), B, H, W, step, 0.0, 3e38, 1.0, 3.0, 1.0, st()),
                   lambda: ops.motion_normal(d0, d1, Q, T, v0, None, w, step=step),
                   lambda: aten_normal(d0, d1, w, v0, Qd, Ad, Td, step),
                   lambda: b_buf.copy_(a_buf))
            launches, op, aten, copy = samples(fns, a.iters, a.warmup)
            got, want = ops.motion_normal(d0, d1, Q, T, v0, None, w, step=step).cpu(), aten_normal(d0, d1, w, v0, Qd, Ad, Td, step)
            Hm, _ = ops.unpack_align_sums(got)
            n = (H // step) * (W // step) * B
            ceiling = 2 * a_buf.numel() * 4 / (copy[0] * 1e-3)
            row = {"frame": [H, W], "B": B, "step": step, "used": [int(v) for v in got[:, 29]], "candidates": [int(v) for v in got[:, 30]],
                   "normal_launches_ms": launches, "motion_normal_ms": op, "aten_normal_ms": aten, "copy_ms": copy,
                   "copy_GBps": round(ceiling / 1e9, 1), "bytes_per_lattice_pixel": 13,
                   "share_of_streaming_ceiling": round(13 * n / ceiling / (launches[0] * 1e-3), 4),
                   "fp64_GFLOPs": round(330 * float(got[:, 29].sum()) / (launches[0] * 1e-3) / 1e9, 1),
                   "aten_over_motion_normal": round(aten[0] / op[0], 2),
                   "max_relative_difference_to_aten": float(((Hm - want[0].cpu()).abs() / want[0].cpu().abs().clamp(min=1e-300)).max()),
                   "counts_equal_to_aten": [int(v) for v in got[:, 29]] == want[4].tolist()}
            rows.append(row)
            print(json.dumps(row), flush=True)
        estimate = {"B": B}
        for step in (1, 2):
            est = ops.motion_estimate(d0, d1, Q, valid0=v0, weight=w, step=step)
            estimate[f"step{step}"] = {"ms": wall(lambda: ops.motion_estimate(d0, d1, Q, valid0=v0, weight=w, step=step), a.frame_iters, 3),
                                       "iterations": est.iterations.tolist(), "converged": est.converged.tolist()}
        rows.append({"motion_estimate": estimate})
        print(json.dumps(estimate), flush=True)
        del a_buf, b_buf
        torch.cuda.empty_cache()
    torch.manual_seed(5)
    model = ecm_amd.get_model("cmfsm").cuda().eval()
    left, right = (torch.randn(1, 3, H, W, device="cuda", generator=g) for _ in range(2))
    eye = torch.eye(4, dtype=F64)
    tracker, odo = models.DisparityTracker(model, Q), models.StereoOdometry(model, Q)
    tracker(left, right)
    odo(left, right)
    o = odo(left, right)
    frame = {"arch": "cmfsm", "frame": [H, W], "B": 1, "iters": a.frame_iters,
             "predict_ms": wall(lambda: model.predict(left, right, (2,)), a.frame_iters, 3),
             "tracker_ms": wall(lambda: tracker(left, right, motion=eye), a.frame_iters, 3),
             "odometry_ms": wall(lambda: odo(left, right), a.frame_iters, 3),
             "odometry_restarted": bool(o.restarted), "odometry_iterations": None if o.estimate is None else o.estimate.iterations.tolist()}
    frame["odometry_minus_tracker_ms"] = round(frame["odometry_ms"][0] - frame["tracker_ms"][0], 4)
    frame["estimator_share_of_frame"] = round(frame["odometry_minus_tracker_ms"] / frame["odometry_ms"][0], 4)
    print(json.dumps(frame), flush=True)
    res = {"what": "ecmm_align_normal_fwd's two launches alone on preallocated buffers, ops.motion_normal with its allocations and its "
                   "host-to-device copy of the matrices, the same sums by ATen on the same tensors, and a device copy of 32 B per pixel; "
                   "each entry [median, lowest, highest] in ms.  motion_estimate and the frames are wall times around a synchronised call "
                   "(they read results on the host).  The frames run the same random-weight cmfsm on one noise pair: the scene does not "
                   "move, so the estimator's iteration count is what that input gives, not a typical one",
           "iters": a.iters, "timing": "device events around each call, alternating inside one loop; wall clock for the host-synchronised ones",
           "rows": rows, "frame": frame}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
