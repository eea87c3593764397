"""torch.autograd.Function skins over the C ABI of libecm_hip.so.

PyTorch is plumbing here (device memory from its caching allocator, the current HIP stream,
autograd bookkeeping); every forward and backward below is a hand-written gfx950 kernel reached
through `_lib.call`.  There is no eager/CPU fallback: a non-CUDA tensor or a missing library raises.
"""
from __future__ import annotations

import collections
import contextlib as _contextlib
import ctypes as C
import dataclasses
import math
import numbers
import os as _os
import random

import torch

from . import _lib

GN_GROUPS = 32
GN_EPS = 1e-5


# ------------------------------------------------------------------------------------ environment switches
# Read once at import; tests and bench.py assign the module attributes afterwards, so every use reads them at call time.
#
# Stride-1 3x3(x3) convolutions -- forward and data gradient -- run on the Winograd F(2x2,3x3) kernel (csrc/conv_wino.hip):
# 2.25x fewer matrix-core multiplies, fp32 throughout.  ECM_WINOGRAD=0 (or ops.WINOGRAD = False) selects the direct
# implicit-GEMM kernels for everything; both are parity-tested.
WINOGRAD = _os.environ.get("ECM_WINOGRAD", "1") != "0"
WINO2D_MIN_CI = int(_os.environ.get("ECM_WINO2D_MIN_CI", "32"))
WINOGRAD_WGRAD = _os.environ.get("ECM_WINOGRAD_WGRAD", "1") != "0"

# Weight gradients on a side stream.  A layer's weight gradient feeds nothing but the optimizer, while its data gradient is on
# the critical path of backward together with the HBM-bound GroupNorm backward passes: launched on a second stream, the
# matrix-bound weight-gradient kernels run under those passes instead of queueing between them (backward at batch 4:
# 86.9 -> 82.3 ms, gradients bit-identical).  Ordering: the side stream waits for the main stream's position at launch (x and
# gy are ready), the operands are recorded on it (the caching allocator must not recycle them under the kernel), and the main
# stream waits for the side stream once per backward pass, from an engine callback that runs when the pass has finished.
# That is safe exactly when nothing reads a weight gradient DURING the pass: it is therefore OFF unless the training harness
# that owns the gradients' consumers turns it on (dist.FlatBucketDDP does: it joins before it gathers) or ECM_WGRAD_OVERLAP=1
# asks for it; non-leaf weights (nn.DataParallel replicas, whose gradients flow on through Broadcast.backward), weights with
# tensor hooks and weights that already HAVE a gradient (a layer used twice in one graph, accumulation over several passes:
# AccumulateGrad then adds on the main stream at once) always stay on the main stream, and so does everything during graph
# capture.  ECM_WGRAD_OVERLAP=0: never.
_WGRAD_ENV = _os.environ.get("ECM_WGRAD_OVERLAP", "")
WGRAD_OVERLAP = _WGRAD_ENV == "1"

# Host run-ahead (round 4).  The operands of a side-stream launch are recorded on that stream, so the caching allocator hands
# their blocks out again only once the side stream's work has FINISHED on the device -- unlike main-stream blocks, which it
# recycles in stream order however far the host runs ahead.  A training loop that never synchronises (the host enqueues a step
# in 23 ms, the device runs it in 124) therefore found none of the previous steps' blocks free and went to the driver for new
# ones every step: 320 hipMalloc calls and 40.7 -> 137.5 GiB reserved over 15 steps, and a step time that depended on how fast
# the driver could hand out memory (2x slower right after another process had released its own: the driver scrubs what it
# hands out again).  So the host waits, at the start of a training forward (models: hot path) and in front of a pass's first side launch, for the
# event recorded behind the PREVIOUS pass's join: at most one step's operands are ever pending, the allocator reaches its steady
# state in the first step, and the device still has the optimiser step + the queued forward to run while the host catches up
# (no bubble: measured step time unchanged on a fresh device).  ECM_WGRAD_PACE=0 turns the wait off (A/B only).
_WGRAD_PACE = _os.environ.get("ECM_WGRAD_PACE", "1") != "0"

# Launch order of a layer's weight gradient and data gradient (see _launch_pair): ECM_WGRAD_FIRST=0 queues the data gradient first.
WGRAD_FIRST = _os.environ.get("ECM_WGRAD_FIRST", "1") == "1"


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host(ctype, values):
    """A HOST array parameter of the ABI (`const int*`, `const float*`, `const float* const*`) as the c_void_p its prototype
    declares; None for values None.  The pointer keeps the array it points into alive."""
    if values is None:
        return None
    values = list(values)
    return C.cast((ctype * len(values))(*values), C.c_void_p)


_CPU_TENSOR = "ecm ops run only on the MI355X HIP path: got a CPU tensor (no CPU fallback exists)"


def _on_device(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(_CPU_TENSOR)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        _on_device(t)
        if t.dtype != torch.float32:
            raise RuntimeError(f"ecm ops are fp32 (got {t.dtype})")


def _need(cond, msg):
    """Operand-shape contract of an op.  The C ABI sees pointers and sizes only: whatever the sizes do not say about a second
    operand has to be established here, BEFORE the launch -- a kernel reading past a smaller tensor is a device fault, not an
    exception.  RuntimeError, as the torch ops these replace raise on mismatched shapes."""
    if not cond:
        raise RuntimeError(msg() if callable(msg) else msg)


def _c(t):
    """Contiguous and 16-byte aligned (the kernels use float4 accesses)."""
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


# ---- the operand contract of the post-processing ops (lr_check .. remap_pair, the check_* functions), stated once.  Parameters
# are refused with ValueError before any tensor is touched; tensors with RuntimeError (_need) before any launch.  Every message
# is formed only when it is raised.
_FLT_MAX = 3.4028234663852886e38


def _is_real(v, bound=None, fp32=False):
    """v is a real number, not a bool, finite (fp32: as an fp32 value too) and, where bound is "> 0" or ">= 0", within it."""
    return not (isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or (fp32 and abs(v) > _FLT_MAX)
                or (bound == "> 0" and v <= 0) or (bound == ">= 0" and v < 0))


def _real(who, name, v, bound=None, fp32=False):
    """v as a float, or ValueError "<who>: <name> <v>: a finite number[ <bound>]"."""
    if not _is_real(v, bound, fp32):
        raise ValueError(f"{who}: {name} {v!r}: a finite number" + (f" {bound}" if bound else ""))
    return float(v)


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _integer(who, name, v, lo, hi=None):
    """v as an int, or ValueError "<who>: <name> <v>: an integer in <lo>..<hi>" (hi None: "an integer >= <lo>")."""
    if not _is_int(v) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{who}: {name} {v!r}: an integer " + (f">= {lo}" if hi is None else f"in {lo}..{hi}"))
    return int(v)


def _bhw(t):
    """A [B,1,H,W] tensor as its [B,H,W] view; any other shape as it is, for the caller's _need to name."""
    return t[:, 0] if t.dim() == 4 and t.shape[1] == 1 else t


def _disp_plane(who, disp, want="want [B,H,W] or [B,1,H,W]"):
    """disp, fp32 on the device, [B,H,W] or [B,1,H,W] and not empty, as its [B,H,W] view."""
    _chk(disp)
    disp = _bhw(disp)
    _need(disp.dim() == 3 and disp.numel() > 0, lambda: f"{who}: disp {tuple(disp.shape)}: {want}")
    return disp


def _plane_like(who, name, t, disp, dtypes, want):
    """t, on the device and of one of `dtypes` (`want` names them), as a [B,H,W] view of the shape of the plane disp."""
    _on_device(t)
    _need(t.dtype in dtypes, lambda: f"{who}: {name} is {t.dtype}: want {want}")
    t = _bhw(t)
    _need(t.shape == disp.shape, lambda: f"{who}: {name} {tuple(t.shape)} against disp {tuple(disp.shape)}")
    return t.detach()


def _mask_plane(who, valid, disp):
    """valid, bool or uint8 of disp's shape, as a contiguous uint8 plane (a bool is one byte, 0 or 1: viewed, not copied)."""
    valid = _plane_like(who, "valid", valid, disp, (torch.bool, torch.uint8), "bool or uint8").contiguous()
    return valid.view(torch.uint8) if valid.dtype == torch.bool else valid


def _guide(who, guide, d):
    """guide [B,C,H,W], C in 1..4 (fp32 on the device: the caller's _chk), against the plane d [B,H,W]: contiguous and aligned."""
    _need(guide.dim() == 4 and guide.shape[0] == d.shape[0] and 1 <= guide.shape[1] <= 4 and guide.shape[2:] == d.shape[1:],
          lambda: f"{who}: guide {tuple(guide.shape)} against disp {tuple(d.shape)}: want [B,C,H,W], C in 1..4")
    return _c(guide.detach())


def _empty_like(t):
    """A CONTIGUOUS uninitialised tensor of t's shape: the kernels write dense row-major buffers, and
    `torch.empty_like` would copy the strides of a non-contiguous `t` (e.g. an einsum output viewed as a weight)."""
    return torch.empty(t.shape, dtype=t.dtype, device=t.device)


def _scratch(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


_SCRATCH = object()      # in an argument list: the place of an entry point's (scratch pointer, scratch bytes) pair


def _call_scratch(device, query, sizes, name, *args, call=None, zero=None):
    """Query `query(*sizes)` for the scratch bytes of entry point `name`, allocate them on `device` and call `name` with
    `args`, the _SCRATCH marker replaced by (pointer, byte count); every other argument is passed through unchanged.
    call: the caller (default _lib.call);  zero: the RuntimeError text for a size query that answers 0 (= unsupported)."""
    nb = _lib.query(query, *sizes)
    if zero is not None and nb == 0:
        raise RuntimeError(zero)
    buf = _scratch(nb, device)
    at = next(i for i, a in enumerate(args) if a is _SCRATCH)
    (call or _lib.call)(name, *args[:at], _p(buf), C.c_longlong(nb), *args[at + 1:])


# ------------------------------------------------------------------------------------ a1 cost volume
class CostVolumeConcat(torch.autograd.Function):
    """cmfsm.py:667-682 -- [B,C,h,w] x2 -> [B,2C,D,h,w]."""

    @staticmethod
    def forward(ctx, left, right, ndisp):
        _chk(left, right)
        _need(left.dim() == 4 and right.shape == left.shape and ndisp >= 1,
              lambda: f"cost_volume: left {tuple(left.shape)}, right {tuple(right.shape)}, ndisp {ndisp}: two [B,C,h,w] maps of one shape")
        left, right = _c(left), _c(right)
        B, Cc, h, w = left.shape
        cost = torch.empty(B, 2 * Cc, ndisp, h, w, device=left.device, dtype=left.dtype)
        _lib.call("ecm_costvol_concat_fwd", _p(left), _p(right), _p(cost), B, Cc, h, w, ndisp, _stream())
        ctx.dims = (B, Cc, h, w, ndisp)
        return cost

    @staticmethod
    def backward(ctx, gcost):
        B, Cc, h, w, D = ctx.dims
        gcost = _c(gcost)
        gl = torch.empty(B, Cc, h, w, device=gcost.device, dtype=gcost.dtype)
        gr = _empty_like(gl)
        _lib.call("ecm_costvol_concat_bwd", _p(gcost), _p(gl), _p(gr), B, Cc, h, w, D, _stream())
        return gl, gr, None


def cost_volume(left, right, ndisp):
    _AGG.guard("cost_volume")
    return CostVolumeConcat.apply(left, right, int(ndisp))


class CostvolConvAssemble(torch.autograd.Function):
    """y[b,co,d,h,x] = P[b,classP(d,x),co,h,x] + Qp[b,classQ(d,x),co,h,x-d+2] (see csrc/costvol_conv.hip);
    backward: gP, gQp = per-class sums of gy over d."""

    @staticmethod
    def forward(ctx, P, Qp, ndisp):
        _chk(P, Qp)
        P, Qp = _c(P), _c(Qp)
        _need(P.dim() == 4 and Qp.dim() == 4, "costvol_conv assemble: P and Qp are [B,classes*Co,h,w(+2)]")
        B, c15, h, w = P.shape
        Co = c15 // 15
        _need(Co >= 1 and c15 == 15 * Co and tuple(Qp.shape) == (B, 6 * Co, h, w + 2) and ndisp >= 2,
              lambda: f"costvol_conv assemble: P {tuple(P.shape)} / Qp {tuple(Qp.shape)} / D {ndisp}: want [B,15Co,h,w], [B,6Co,h,w+2], D >= 2")
        y = torch.empty(B, Co, ndisp, h, w, device=P.device, dtype=P.dtype)
        _lib.call("ecm_costvol_conv_assemble_fwd", _p(P), _p(Qp), _p(y), B, Co, ndisp, h, w, _stream())
        ctx.dims = (B, Co, ndisp, h, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, Co, D, h, w = ctx.dims
        gy = _c(gy)
        gP = torch.empty(B, 15 * Co, h, w, device=gy.device, dtype=gy.dtype)
        gQ = torch.empty(B, 6 * Co, h, w + 2, device=gy.device, dtype=gy.dtype)
        _lib.call("ecm_costvol_conv_assemble_bwd", _p(gy), _p(gP), _p(gQ), B, Co, D, h, w, _stream())
        return gP, gQ, None


class ClassWeights(torch.autograd.Function):
    """dres0[0][0].weight [Co,2C,3,3,3] -> (wP [15*Co,C,3,3], wQ [6*Co,C,3,5]): the class-indexed 2-D kernels of the collapsed
    first convolution (csrc/costvol_conv.hip).  Class = which taps pass the wedge `x >= d` of cmfsm.py:678-679 and the depth
    padding: reference half (clamp(d-x,-2,2)+2)*3 + edge with edge = 0 / 1 / 2 for the first / an interior / the last
    disparity plane; target half edge*2 + (x == w-1), a passing tap landing on column kw-kd+2 of the sheared 3x5 kernel."""

    @staticmethod
    def forward(ctx, w):
        _chk(w)
        _need(w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and w.shape[1] % 2 == 0,
              lambda: f"class weights: w {tuple(w.shape)}: want the first 3x3x3 convolution's [Co,2C,3,3,3]")
        w = _c(w)
        Co, C2 = w.shape[:2]
        Cc = C2 // 2
        wP = torch.empty(15 * Co, Cc, 3, 3, device=w.device, dtype=w.dtype)
        wQ = torch.empty(6 * Co, Cc, 3, 5, device=w.device, dtype=w.dtype)
        _lib.call("ecm_costvol_class_weights_fwd", _p(w), _p(wP), _p(wQ), Co, Cc, _stream())
        ctx.dims = (Co, Cc)
        return wP, wQ

    @staticmethod
    def backward(ctx, gwP, gwQ):
        Co, Cc = ctx.dims
        gw = torch.empty(Co, 2 * Cc, 3, 3, 3, device=gwP.device, dtype=gwP.dtype)
        _lib.call("ecm_costvol_class_weights_bwd", _p(_c(gwP)), _p(_c(gwQ)), _p(gw), Co, Cc, _stream())
        return gw


def costvol_conv3d(left, right, weight, ndisp):
    """conv3d(cost_volume(left, right, ndisp), weight, stride 1, pad 1)  (cmfsm.py:667-684) WITHOUT the 4-D volume: both
    halves of the concat volume are constant along a line in (d, x), so the 3x3x3 convolution collapses to class-indexed
    2-D convolutions of the two feature maps (3x3 on `left`, sheared 3x5 on `right`) -- see csrc/costvol_conv.hip.
    weight: [Co, 2C, 3, 3, 3] (the reference's dres0[0][0].weight)."""
    _AGG.guard("costvol_conv3d")
    _chk(left, right, weight)                  # before ClassWeights launches anything
    _need(left.dim() == 4 and right.shape == left.shape and weight.dim() == 5,
          lambda: f"costvol_conv3d: left {tuple(left.shape)}, right {tuple(right.shape)}, weight {tuple(weight.shape)}")
    Cc = left.shape[1]
    if weight.shape[1] != 2 * Cc or ndisp < 2:
        return conv3d_k3(cost_volume(left, right, ndisp), weight, 1)
    wP, wQ = ClassWeights.apply(weight)
    h, w = left.shape[-2:]
    P = conv2d(left, wP, 1, 1, 1, 1, h, w)                      # 3x3, pad 1                                  [B,15Co,h,w]
    # sheared 3x5 on the target features with 2 extra zero columns on the left: pad (1, 2) of F.pad(right, (2, 0)) is a
    # left padding of 4 and a right padding of 2 -> output width w + 2                                        [B,6Co,h,w+2]
    Qp = conv2d(right, wQ, 1, 1, 1, 4, h, w + 2)
    return CostvolConvAssemble.apply(P, Qp, int(ndisp))


# ------------------------------------------------------------------------------------ a8 soft-argmin
class SoftArgminHeads(torch.autograd.Function):
    """c [NH,B,D,h,w] raw classifier outputs -> disp [NH,B,h,w]; head k uses logits c_0+...+c_k
    (cmfsm.py:703-706, 725-728, 748-753)."""

    @staticmethod
    def forward(ctx, c):
        _chk(c)
        _need(c.dim() == 5 and c.numel() > 0, lambda: f"softargmin_heads: c {tuple(c.shape)}: want [heads,B,D,h,w]")
        c = _c(c)
        NH, B, D, h, w = c.shape
        disp = torch.empty(NH, B, h, w, device=c.device, dtype=c.dtype)
        _lib.call("ecm_softargmin_heads_fwd", _p(c), C.c_longlong(B * D * h * w), _p(disp), NH, B, D, h * w, _stream())
        ctx.save_for_backward(c)
        return disp

    @staticmethod
    def backward(ctx, gdisp):
        (c,) = ctx.saved_tensors
        NH, B, D, h, w = c.shape
        gdisp = _c(gdisp)
        gc = _empty_like(c)
        _lib.call("ecm_softargmin_heads_bwd", _p(c), C.c_longlong(B * D * h * w), _p(gdisp), _p(gc), NH, B, D, h * w,
                  _stream())
        return gc


def softargmin_heads(c):
    return SoftArgminHeads.apply(c)


def disparity_regression(x):
    """disparityregression.forward (cmfsm.py:120-123): [B,D,h,w] probabilities -> [B,h,w]. Forward only."""
    _chk(x)
    _need(x.dim() == 4 and x.numel() > 0, lambda: f"disparity_regression: x {tuple(x.shape)}: want [B,D,h,w]")
    x = _c(x)
    B, D, h, w = x.shape
    out = torch.empty(B, h, w, device=x.device, dtype=x.dtype)
    _lib.call("ecm_disparity_regression_fwd", _p(x), _p(out), B, D, h * w, _stream())
    return out


# ------------------------------------------------------------------------------------ a9 aggregation
class ECMAggregate9(torch.autograd.Function):
    """d [NH,B,h,w], w9 [B,9,H,W] -> [NH,B,H,W]   (cmfsm.py:709-723)."""

    @staticmethod
    def forward(ctx, d, w9, scale):
        _chk(d, w9)
        d, w9 = _c(d), _c(w9)
        _need(d.dim() == 4 and scale >= 1, lambda: f"ecm_aggregate9: d {tuple(d.shape)}, scale {scale}: want [heads,B,h,w]")
        NH, B, h, w = d.shape
        _need(tuple(w9.shape) == (B, 9, h * scale, w * scale),
              lambda: f"ecm_aggregate9: w9 {tuple(w9.shape)} for d {tuple(d.shape)} at scale {scale}: want [B,9,h*scale,w*scale]")
        out = torch.empty(NH, B, h * scale, w * scale, device=d.device, dtype=d.dtype)
        _lib.call("ecm_aggregate9_fwd", _p(d), _p(w9), _p(out), NH, B, h, w, scale, _stream())
        ctx.save_for_backward(d, w9)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, gout):
        d, w9 = ctx.saved_tensors
        NH, B, h, w = d.shape
        gout = _c(gout)
        gd, gw9 = _empty_like(d), _empty_like(w9)
        _lib.call("ecm_aggregate9_bwd", _p(d), _p(w9), _p(gout), _p(gd), _p(gw9), NH, B, h, w, ctx.scale, _stream())
        return gd, gw9, None


def ecm_aggregate9(d, w9, scale):
    return ECMAggregate9.apply(d, w9, int(scale))


# ------------------------------------------------------------------------------------ a3 ECM weights
_ECM_MLP_SIZES = (2112, 512, 128, 8)      # similarity_measure1's four 1x1 kernels: 66->32, 32->16, 16->8, 8->1
_VARIANT_PLANES = {0: 9, 1: 5, 2: 3}


class ContextWeights(torch.autograd.Function):
    """Context-mapping weights: variant 0 eight_related (cmfsm.py:431-593), 1/2 six_related on the reference / target
    image (cmfsm_sub_8.py:440-572).  lr [B,32,h,w], hr [B,32,H,W] -> [B,N,H,W] with N = 9, 5, 3.
    Variant 0 goes through the entry points it was introduced under (ecm_weights9_fwd / _bwd: thin wrappers of
    ecm_context_weights_* in the library, and the names the benchmark's timers key on)."""

    @staticmethod
    def forward(ctx, lr, hr, W0, W1, W2, W3, variant):
        _chk(lr, hr, W0, W1, W2, W3)
        _need(lr.dim() == 4 and hr.dim() == 4 and hr.shape[0] == lr.shape[0] and lr.shape[-1] > 0 and lr.shape[-2] > 0,
              lambda: f"context weights: lr {tuple(lr.shape)}, hr {tuple(hr.shape)}: want [B,32,h,w] and [B,32,H,W]")
        _need((W0.numel(), W1.numel(), W2.numel(), W3.numel()) == _ECM_MLP_SIZES,
              lambda: f"context weights: the similarity MLP's kernels hold {_ECM_MLP_SIZES} values (cmfsm.py:400-427), got "
                      f"{(W0.numel(), W1.numel(), W2.numel(), W3.numel())}")
        lr, hr = _c(lr), _c(hr)
        W0, W1, W2, W3 = (_c(t) for t in (W0, W1, W2, W3))
        B, Cc, h, w = lr.shape
        H, W = hr.shape[-2:]
        s = W // w
        if s % 2 != 0:
            raise ValueError("odd scale between hr and lr features (the reference calls exit() here"
                             + (", cmfsm.py:448-449)" if variant == 0 else ")"))
        if Cc != 32 or hr.shape[1] != 32 or H != h * s or W != w * s:
            raise RuntimeError(f"{'ecm_weights9' if variant == 0 else 'context_weights'}: unsupported shapes "
                               f"lr {tuple(lr.shape)} hr {tuple(hr.shape)}")
        _need(variant in _VARIANT_PLANES, lambda: f"context weights: variant {variant} (0 eight-related, 1 / 2 six-related)")
        if variant == 0 and s != 4:   # matrix_generation hard-codes scale 4 (cmfsm.py:392): the reference's forward fails in torch.cat otherwise
            raise RuntimeError(f"eight_related_context_mapping exists at scale 4 only (got {s}): the reference's offset tables "
                               "are 4 x 4 and its forward raises a shape error at any other scale")
        out = torch.empty(B, _VARIANT_PLANES[variant], H, W, device=lr.device, dtype=lr.dtype)
        name, tail = ("ecm_weights9_fwd", (s,)) if variant == 0 else ("ecm_context_weights_fwd", (s, variant))
        _call_scratch(lr.device, "ecm_weights9_scratch_bytes", (B, h, w), name, _p(lr), _p(hr), _p(W0), _p(W1), _p(W2), _p(W3),
                      _p(out), _SCRATCH, B, h, w, *tail, _stream())
        ctx.save_for_backward(lr, hr, W0, W1, W2, W3, out)
        ctx.s, ctx.variant = s, variant
        return out

    @staticmethod
    def backward(ctx, g):
        lr, hr, W0, W1, W2, W3, out = ctx.saved_tensors
        B, _, h, w = lr.shape
        s, variant = ctx.s, ctx.variant
        g = _c(g)
        glr, ghr = _empty_like(lr), _empty_like(hr)
        gW = torch.empty(sum(_ECM_MLP_SIZES), device=lr.device, dtype=lr.dtype)
        if variant == 0:
            query, name, tail, zero = "ecm_weights9_bwd_scratch_bytes", "ecm_weights9_bwd", (s,), None
        else:
            query, name, tail = "ecm_context_weights_bwd_scratch_bytes", "ecm_context_weights_bwd", (s, variant)
            zero = f"context_weights backward: unsupported scale {s} (the registered architectures' scales are 4, 8, 16)"
        _call_scratch(lr.device, query, (B, h, w) + tail, name, _p(lr), _p(hr), _p(W0), _p(W1), _p(W2), _p(W3),
                      _p(out), _p(g), _p(glr), _p(ghr), _p(gW), _SCRATCH, B, h, w, *tail, _stream(), zero=zero)
        return (glr, ghr, gW[:2112].view_as(W0), gW[2112:2624].view_as(W1), gW[2624:2752].view_as(W2),
                gW[2752:].view_as(W3), None)


def context_weights(lr, hr, W0, W1, W2, W3, variant):
    return ContextWeights.apply(lr, hr, W0, W1, W2, W3, int(variant))


def ecm_weights9(lr, hr, W0, W1, W2, W3):
    """eight_related_context_mapping (cmfsm.py:443-593): lr [B,32,h,w], hr [B,32,H,W] -> w9 [B,9,H,W]."""
    return ContextWeights.apply(lr, hr, W0, W1, W2, W3, 0)


# The operand contract of a head family, stated once: the plain op's Function.forward and the family's _stats and _mode ops all
# go through it, under their own name `who`.  Refusals come in one order -- device and dtype, c and the sizes, the mode radius
# (where one is given), then, with the operands contiguous, the other tensors' shapes -- and all before any launch.  Each
# returns the contiguous operands, the sizes (NH, B, Dl, h, w, H, W), the head stride of c and the checked radius.
_NO_RADIUS = object()      # the op takes no mode radius


def _volume_operands(who, c, m5, mt3, scale, radius=_NO_RADIUS):
    _chk(c, m5, mt3)
    _need(c.dim() == 5 and scale >= 1 and c.numel() > 0, lambda: f"{who}: c {tuple(c.shape)}, scale {scale}")
    if radius is not _NO_RADIUS:
        radius = check_mode_radius(radius)
    c, m5, mt3 = _c(c), _c(m5), _c(mt3)
    NH, B, Dl, h, w = c.shape
    H, W = h * scale, w * scale
    _need(tuple(m5.shape) == (B, 5, H, W) and tuple(mt3.shape) == (B, 3, H, W),
          lambda: f"{who}: m5 {tuple(m5.shape)} / mt3 {tuple(mt3.shape)} for c {tuple(c.shape)} at scale {scale}: "
                  "want [B,5,h*scale,w*scale] and [B,3,h*scale,w*scale]")
    return (c, m5, mt3), (NH, B, Dl, h, w, H, W), C.c_longlong(B * Dl * h * w), radius


def _trilinear_operands(who, c, Do, H, W, radius=_NO_RADIUS):
    _chk(c)
    _need(c.dim() == 5 and c.numel() > 0 and Do >= 1 and H >= 1 and W >= 1,
          lambda: f"{who}: c {tuple(c.shape)} -> ({Do}, {H}, {W})")
    if radius is not _NO_RADIUS:
        radius = check_mode_radius(radius)
    c = _c(c)
    NH, B, Dl, h, w = c.shape
    return c, (NH, B, Dl, h, w, H, W), C.c_longlong(B * Dl * h * w), radius


def _eight_operands(kind, c, w9, scale, radius=_NO_RADIUS):
    """Of ecm_aggregate9_<kind>.  Also launches the head's first kernel, the column softmax that stores its normalisers:
    -> ..., d, lse [NH,B,h,w]."""
    who = f"ecm_aggregate9_{kind}"
    _chk(c, w9)
    _need(c.dim() == 5 and c.numel() > 0 and scale >= 1, lambda: f"{who}: c {tuple(c.shape)}, scale {scale}: want [heads,B,D,h,w]")
    if radius is not _NO_RADIUS:
        radius = check_mode_radius(radius, scale)
    c, w9 = _c(c), _c(w9)
    NH, B, D, h, w = c.shape
    H, W = h * scale, w * scale
    _need(tuple(w9.shape) == (B, 9, H, W),
          lambda: f"{who}: w9 {tuple(w9.shape)} for c {tuple(c.shape)} at scale {scale}: want [B,9,h*scale,w*scale]")
    d = torch.empty(NH, B, h, w, device=c.device, dtype=c.dtype)
    lse = torch.empty(NH, B, h, w, device=c.device, dtype=c.dtype)
    hs = C.c_longlong(B * D * h * w)
    _lib.call("ecm_softargmin_heads_lse_fwd", _p(c), hs, _p(d), _p(lse), NH, B, D, h * w, _stream())
    return (c, w9), (NH, B, D, h, w, H, W), hs, radius, d, lse


def _head_out(c, sizes, planes=None):
    """[NH,B,H,W], or the [NH,planes,B,H,W] of a stats / modal buffer, beside c."""
    NH, B, H, W = sizes[0], sizes[1], sizes[5], sizes[6]
    return torch.empty((NH, B, H, W) if planes is None else (NH, planes, B, H, W), device=c.device, dtype=c.dtype)


class VolumeMapping(torch.autograd.Function):
    """Fused volume-mapping head (cmfsm_sub_16.py:767-801): c [NH,B,Dl,h,w], m5 [B,5,H,W], mt3 [B,3,H,W] -> [NH,B,H,W]."""

    @staticmethod
    def forward(ctx, c, m5, mt3, scale):
        (c, m5, mt3), sizes, hs, _ = _volume_operands("volume_mapping", c, m5, mt3, scale)
        out = _head_out(c, sizes)
        _lib.call("ecm_volume_mapping_fwd", _p(c), hs, _p(m5), _p(mt3), _p(out), *sizes[:5], scale, _stream())
        ctx.save_for_backward(c, m5, mt3)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        c, m5, mt3 = ctx.saved_tensors
        NH, B, Dl, h, w = c.shape
        g = _c(g)
        gc, gm5, gmt3 = _empty_like(c), _empty_like(m5), _empty_like(mt3)
        _call_scratch(c.device, "ecm_volume_mapping_bwd_scratch_bytes", (NH, B, Dl, h, w, ctx.scale), "ecm_volume_mapping_bwd",
                      _p(c), C.c_longlong(B * Dl * h * w), _p(m5), _p(mt3), _p(g), _p(gc), _p(gm5), _p(gmt3), _SCRATCH,
                      NH, B, Dl, h, w, ctx.scale, _stream())
        return gc, gm5, gmt3, None


def volume_mapping(c, m5, mt3, scale):
    return VolumeMapping.apply(c, m5, mt3, int(scale))


class TrilinearSoftArgmin(torch.autograd.Function):
    """Fused trilinear head (bilinear_cmf.py:447-471): c [NH,B,Dl,h,w] -> [NH,B,H,W]."""

    @staticmethod
    def forward(ctx, c, Do, H, W):
        c, sizes, hs, _ = _trilinear_operands("trilinear_softargmin", c, Do, H, W)
        out = _head_out(c, sizes)
        _lib.call("ecm_trilinear_softargmin_fwd", _p(c), hs, _p(out), *sizes[:5], Do, H, W, _stream())
        ctx.save_for_backward(c)
        ctx.dims = (Do, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        (c,) = ctx.saved_tensors
        NH, B, Dl, h, w = c.shape
        Do, H, W = ctx.dims
        g = _c(g)
        gc = _empty_like(c)
        _call_scratch(c.device, "ecm_trilinear_softargmin_bwd_scratch_bytes", (NH, B, Dl, h, w, H, W),
                      "ecm_trilinear_softargmin_bwd", _p(c), C.c_longlong(B * Dl * h * w), _p(g), _p(gc), _SCRATCH,
                      NH, B, Dl, h, w, Do, H, W, _stream())
        return gc, None, None, None


def trilinear_softargmin(c, Do, H, W):
    return TrilinearSoftArgmin.apply(c, int(Do), int(H), int(W))


# ------------------------------------------------------------------------------------ per-pixel uncertainty of the heads
# DESIGN.md section 15.  Forward only: each op returns (disp, std, peak, entropy), every one [NH,B,H,W] and outside any graph;
# disp is bit-identical to the plain head's, the other three describe the distribution whose mean it is.
def _stats_planes(disp, stats):
    return disp, stats[:, 0], stats[:, 1], stats[:, 2]


@torch.no_grad()
def ecm_aggregate9_stats(c, w9, scale):
    """The eight-neighbour head (softargmin_heads + ecm_aggregate9) on c [NH,B,D,h,w] raw classifier outputs and w9 [B,9,H,W],
    with the statistics of each HR pixel's mixture of its valid neighbours' low-resolution distributions."""
    scale = int(scale)
    (c, w9), sizes, hs, _, d, lse = _eight_operands("stats", c.detach(), w9.detach(), scale)
    NH, B, D, h, w = sizes[:5]
    disp, stats = _head_out(c, sizes), _head_out(c, sizes, 3)
    _lib.call("ecm_aggregate9_fwd", _p(d), _p(w9), _p(disp), NH, B, h, w, scale, _stream())
    _lib.call("ecm_aggregate9_stats_fwd", _p(c), hs, _p(lse), _p(w9), _p(stats), NH, B, D, h, w, scale, _stream())
    return _stats_planes(disp, stats)


@torch.no_grad()
def volume_mapping_stats(c, m5, mt3, scale):
    """volume_mapping with the statistics of its softmax over the Dl * scale fused logits."""
    scale = int(scale)
    (c, m5, mt3), sizes, hs, _ = _volume_operands("volume_mapping_stats", c.detach(), m5.detach(), mt3.detach(), scale)
    disp, stats = _head_out(c, sizes), _head_out(c, sizes, 3)
    _lib.call("ecm_volume_mapping_stats_fwd", _p(c), hs, _p(m5), _p(mt3), _p(disp), _p(stats), *sizes[:5], scale, _stream())
    return _stats_planes(disp, stats)


@torch.no_grad()
def trilinear_softargmin_stats(c, Do, H, W):
    """trilinear_softargmin with the statistics of its softmax over the Do interpolated logits."""
    Do, H, W = int(Do), int(H), int(W)
    c, sizes, hs, _ = _trilinear_operands("trilinear_softargmin_stats", c.detach(), Do, H, W)
    disp, stats = _head_out(c, sizes), _head_out(c, sizes, 3)
    _lib.call("ecm_trilinear_softargmin_stats_fwd", _p(c), hs, _p(disp), _p(stats), *sizes[:5], Do, H, W, _stream())
    return _stats_planes(disp, stats)


# ------------------------------------------------------------------------------------ modal disparity of the heads
# DESIGN.md section 16.  Forward only: each op returns (mode, mass, index), every one [NH,B,H,W] and outside any graph, of the
# distribution p whose mean the head returns: index the highest level of p in full-resolution pixels (lowest on an exact tie),
# mass the share of p within `radius` pixels of it, mode p's mean inside that window.  The disparity itself is the plain op's.
def check_mode_radius(radius, scale=1):
    """radius as an int: a non-negative integer number of full-resolution pixels, a multiple of `scale` where the levels of p
    are `scale` pixels apart (the eight-neighbour head)."""
    if not _is_int(radius):
        raise ValueError(f"mode radius {radius!r}: an integer number of full-resolution pixels")
    radius = int(radius)
    if radius < 0:
        raise ValueError(f"mode radius {radius}: must be >= 0")
    if radius % scale:
        raise ValueError(f"mode radius {radius}: the levels of this head's distribution are {scale} pixels apart, so the radius "
                         f"must be a multiple of {scale}")
    return radius


def _mode_planes(modal):
    return modal[:, 0], modal[:, 1], modal[:, 2]


@torch.no_grad()
def ecm_aggregate9_mode(c, w9, scale, radius):
    """(mode, mass, index) of each HR pixel's mixture of its valid neighbours' low-resolution distributions (the operands of
    ecm_aggregate9_stats); radius must be a multiple of scale."""
    scale = int(scale)
    (c, w9), sizes, hs, radius, _, lse = _eight_operands("mode", c.detach(), w9.detach(), scale, radius)
    modal = _head_out(c, sizes, 3)
    _lib.call("ecm_aggregate9_mode_fwd", _p(c), hs, _p(lse), _p(w9), _p(modal), *sizes[:5], scale, radius, _stream())
    return _mode_planes(modal)


@torch.no_grad()
def volume_mapping_mode(c, m5, mt3, scale, radius):
    """(mode, mass, index) of volume_mapping's softmax over the Dl * scale fused logits."""
    scale = int(scale)
    (c, m5, mt3), sizes, hs, radius = _volume_operands("volume_mapping_mode", c.detach(), m5.detach(), mt3.detach(), scale,
                                                       radius)
    modal = _head_out(c, sizes, 3)
    _lib.call("ecm_volume_mapping_mode_fwd", _p(c), hs, _p(m5), _p(mt3), _p(modal), *sizes[:5], scale, radius, _stream())
    return _mode_planes(modal)


@torch.no_grad()
def trilinear_softargmin_mode(c, Do, H, W, radius):
    """(mode, mass, index) of trilinear_softargmin's softmax over the Do interpolated logits."""
    Do, H, W = int(Do), int(H), int(W)
    c, sizes, hs, radius = _trilinear_operands("trilinear_softargmin_mode", c.detach(), Do, H, W, radius)
    modal = _head_out(c, sizes, 3)
    _lib.call("ecm_trilinear_softargmin_mode_fwd", _p(c), hs, _p(modal), *sizes[:5], Do, H, W, radius, _stream())
    return _mode_planes(modal)


# ------------------------------------------------------------------------------------ left-right consistency check
# DESIGN.md section 17.  Forward only, one kernel: the error of the left disparity against the right view's disparity warped
# into the left view, the failure class and the disparity filled from the background.
LR_KINDS = ("consistent", "occluded", "mismatch", "out of view")      # the values 0..3 of the kind plane


def lr_check_max_width():
    """The widest map lr_check takes (a size query of the library: no GPU needed)."""
    return int(_lib.query("ecm_lr_check_max_width"))


def check_lr_tolerances(threshold, rel):
    """(threshold, rel) as floats: both finite and >= 0 (pixels; a share of the disparity)."""
    return _real("lr_check", "threshold", threshold, ">= 0"), _real("lr_check", "rel", rel, ">= 0")


@torch.no_grad()
def lr_check(disp_l, disp_r, threshold=1.0, rel=0.0, mirrored=False, with_source=False):
    """(error, kind, filled[, src]) of the left-right cross-check, each [B,H,W]: disp_l the left view's disparity, disp_r the
    right view's in right-image coordinates ([B,H,W] or [B,1,H,W], pixels); mirrored: disp_r is stored flipped along W, as
    forward(flip(right), flip(left)) returns it.  A pixel is consistent (kind 0) where |d - r| <= max(threshold, rel * d), r the
    right disparity interpolated at x - d; else occluded (1) where r > d, else a mismatch (2); out of view (3) where x - d
    leaves the image or d is not finite.  error is |d - r| (+inf for kind 3 and a non-finite r), kind a float plane, filled d
    where consistent and elsewhere the smaller of the nearest consistent disparities on the row's left and right (0 if the row
    has none); src (int32, with_source=True) the column it came from, -1 for none."""
    threshold, rel = check_lr_tolerances(threshold, rel)               # before any device work
    _chk(disp_l, disp_r)
    disp_l, disp_r = _bhw(disp_l), _bhw(disp_r)
    _need(disp_l.dim() == 3 and disp_l.numel() > 0 and disp_r.shape == disp_l.shape,
          lambda: f"lr_check: disp_l {tuple(disp_l.shape)}, disp_r {tuple(disp_r.shape)}: want two equal [B,H,W] or [B,1,H,W]")
    B, H, W = disp_l.shape
    dl, dr = _c(disp_l.detach()), _c(disp_r.detach())
    check = torch.empty(3, B, H, W, device=dl.device, dtype=dl.dtype)
    src = torch.empty(B, H, W, device=dl.device, dtype=torch.int32) if with_source else None
    # W beyond lr_check_max_width() is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecm_lr_check_fwd", _p(dl), _p(dr), _p(check), _p(src), B, H, W, threshold, rel, int(bool(mirrored)), _stream())
    return (check[0], check[1], check[2]) + ((src,) if with_source else ())


# ------------------------------------------------------------------------------------ disparity post-filters
# DESIGN.md section 18.  Forward only, one kernel each: the masked lower median of a (2r+1)^2 window, and the joint bilateral
# filter guided by an image.  A sample is usable iff it is inside the image, finite and valid; windows are clipped to the image.
DISP_FILTER_KINDS = ("median", "bilateral")                            # the `kind` of ecm_disp_filter_max_radius: 0, 1


def disp_filter_max_radius(kind):
    """The largest radius of disparity_median ("median") or disparity_bilateral ("bilateral"): a size query, no GPU needed."""
    if kind not in DISP_FILTER_KINDS:
        raise ValueError(f"disp_filter_max_radius: kind {kind!r}: one of {DISP_FILTER_KINDS}")
    return int(_lib.query("ecm_disp_filter_max_radius", DISP_FILTER_KINDS.index(kind)))


def _check_filter_radius(who, kind, radius):
    return _integer(who, "radius", radius, 1, disp_filter_max_radius(kind))


def check_median_radius(radius, who="disparity_median"):
    """radius as an int: 1, 2 or 3 (a 3x3, 5x5 or 7x7 window)."""
    return _check_filter_radius(who, "median", radius)


def check_bilateral_parameters(radius, sigma_space, sigma_color, who="disparity_bilateral"):
    """(radius, sigma_space, sigma_color): an int in 1..disp_filter_max_radius("bilateral") and two finite floats > 0."""
    return (_check_filter_radius(who, "bilateral", radius), _real(who, "sigma_space", sigma_space, "> 0"),
            _real(who, "sigma_color", sigma_color, "> 0"))


def _filter_planes(who, disp, valid):
    """disp as a contiguous [B,H,W] plane and valid as a contiguous uint8 plane of the same shape (or None)."""
    disp = _disp_plane(who, disp)
    return _c(disp.detach()), None if valid is None else _mask_plane(who, valid, disp)


@torch.no_grad()
def disparity_median(disp, valid=None, radius=2, with_support=False):
    """The masked lower median of disp ([B,H,W] or [B,1,H,W], pixels) over a (2 radius + 1)^2 window clipped to the image, as a
    [B,H,W] plane: the value of rank floor((m-1)/2) among the m usable samples of the window -- inside the image, finite, and
    valid != 0 (valid: bool or uint8 of disp's shape; None: all ones) -- so one of the inputs bit for bit, and 0 where m == 0.
    with_support=True returns (median, support), support = m as a float plane.  radius 1, 2 or 3."""
    radius = check_median_radius(radius)                               # before any device work
    d, v = _filter_planes("disparity_median", disp, valid)
    B, H, W = d.shape
    out = torch.empty(2, B, H, W, device=d.device, dtype=d.dtype)
    # B * H * W >= 2^31 is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecm_disp_median_fwd", _p(d), _p(v), _p(out), B, H, W, radius, _stream())
    return (out[0], out[1]) if with_support else out[0]


@torch.no_grad()
def disparity_bilateral(disp, guide, valid=None, radius=4, sigma_space=2.0, sigma_color=0.25, with_weight=False):
    """The joint bilateral filter of disp ([B,H,W] or [B,1,H,W]) guided by guide [B,C,H,W] (C in 1..4, fp32; e.g. the left image
    as the model consumes it), as a [B,H,W] plane: sum w d / sum w over the usable samples q of the (2 radius + 1)^2 window
    clipped to the image, w = exp(-|q - p|^2 / (2 sigma_space^2) - |guide[p] - guide[q]|^2 / (2 sigma_color^2)); a sample whose
    exponent is NaN is left out; 0 where sum w == 0.  A pixel that is not usable itself is written from its neighbours (hole
    filling).  with_weight=True returns (refined, weight), weight = sum w.  radius in 1..disp_filter_max_radius("bilateral")."""
    radius, sigma_space, sigma_color = check_bilateral_parameters(radius, sigma_space, sigma_color)      # before any device work
    _chk(guide)
    d, v = _filter_planes("disparity_bilateral", disp, valid)
    B, H, W = d.shape
    g = _guide("disparity_bilateral", guide, d)
    out = torch.empty(2, B, H, W, device=d.device, dtype=d.dtype)
    _lib.call("ecm_disp_bilateral_fwd", _p(d), _p(v), _p(g), _p(out), B, g.shape[1], H, W, radius, sigma_space, sigma_color, _stream())
    return (out[0], out[1]) if with_weight else out[0]


# ------------------------------------------------------------------------------------ speckle filter
# DESIGN.md section 19.  Forward only: the connected segments of near-constant disparity (4-neighbours, both usable,
# |d[p] - d[q]| <= max_diff), each pixel's segment label and size, and the map with the segments of at most max_size pixels removed.
def check_speckle_parameters(max_size, max_diff, who="disparity_speckle"):
    """(max_size, max_diff) as an int and a float: an integer >= 0 (pixels) and a finite number >= 0 (pixels of disparity)."""
    return _integer(who, "max_size", max_size, 0), _real(who, "max_diff", max_diff, ">= 0")


@torch.no_grad()
def disparity_speckle(disp, valid=None, max_size=200, max_diff=1.0, with_segments=False):
    """The speckle filter of disp ([B,H,W] or [B,1,H,W], pixels) as a [B,H,W] plane: disp, bit for bit, where the pixel is usable
    -- finite, and valid != 0 (valid: bool or uint8 of disp's shape; None: all ones) -- and its segment has more than max_size
    pixels; 0 elsewhere.  A segment is a connected component of the usable pixels under "4-neighbours in the same image whose
    disparities differ by at most max_diff" (fp32, inclusive; OpenCV's filterSpeckles rule, a segment of exactly max_size pixels
    is removed).  with_segments=True returns (out, label, size), both int32: the row-major index y*W + x, within its image, of
    the segment's first pixel (-1 where not usable) and the segment's pixel count (0 where not usable).  The defaults (200 pixels,
    1.0) are the values customary with OpenCV; their effect on EPE or D1 has not been measured."""
    max_size, max_diff = check_speckle_parameters(max_size, max_diff)  # before any device work
    d, v = _filter_planes("disparity_speckle", disp, valid)
    B, H, W = d.shape
    out = torch.empty(B, H, W, device=d.device, dtype=d.dtype)
    segments = torch.empty(2, B, H, W, device=d.device, dtype=torch.int32)
    # B * H * W >= 2^31 is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecm_disp_speckle_fwd", _p(d), _p(v), _p(out), _p(segments), B, H, W, max_size, max_diff, _stream())
    return (out, segments[0], segments[1]) if with_segments else out


# ------------------------------------------------------------------------------------ WLS smoother
# DESIGN.md section 20.  Forward only: the confidence-weighted fast global smoother (OpenCV's DisparityWLSFilter), 2T launches.
WLS_MAX_ITERATIONS = 8


def check_wls_parameters(lam, sigma_color, iterations, who="disparity_wls"):
    """(lam, sigma_color, iterations): two finite floats > 0 and an int in 1..8."""
    return (_real(who, "lam", lam, "> 0"), _real(who, "sigma_color", sigma_color, "> 0"),
            _integer(who, "iterations", iterations, 1, WLS_MAX_ITERATIONS))


@torch.no_grad()
def disparity_wls(disp, guide, confidence=None, lam=8000.0, sigma_color=0.25, iterations=3, with_weight=False):
    """The WLS smoothing of disp ([B,H,W] or [B,1,H,W], pixels) guided by guide [B,C,H,W] (C in 1..4, fp32; e.g. the left image as
    the model consumes it), as a [B,H,W] plane: N = confidence * disp and D = confidence each go through `iterations` rounds of
    "every row, then every column" of the tridiagonal solve (I + lam_t A) u = f, A the Laplacian of the link weights
    w = exp(-|guide[p] - guide[q]| / sigma_color) between 4-neighbours (a NaN weight cuts the link) and lam_t =
    1.5 * 4^(T-t) / (4^T - 1) * lam; the result is N / D where D > 0 and 0 elsewhere.  confidence: a float plane of disp's shape
    (bool or uint8 is converted; None: all ones); a pixel whose disp is not finite, or whose confidence is not finite or is
    negative, counts as confidence 0 -- holes need no filling.  with_weight=True returns (smoothed, weight), weight = D.
    The defaults (8000, 3: customary with OpenCV; 0.25: the bilateral filter's) are untested for quality."""
    lam, sigma_color, iterations = check_wls_parameters(lam, sigma_color, iterations)            # before any device work
    _chk(guide)
    d, _ = _filter_planes("disparity_wls", disp, None)
    B, H, W = d.shape
    conf = confidence
    if conf is not None:
        conf = _c(_plane_like("disparity_wls", "confidence", conf, d, (torch.float32, torch.bool, torch.uint8),
                              "float32, bool or uint8").to(torch.float32))
    g = _guide("disparity_wls", guide, d)
    out = torch.empty(2, B, H, W, device=d.device, dtype=d.dtype)
    scratch = _scratch(_lib.query("ecm_disp_wls_scratch_bytes", B, H, W), d.device)
    # B * H * W >= 2^31 is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecm_disp_wls_fwd", _p(d), _p(conf), _p(g), _p(out), _p(scratch), B, g.shape[1], H, W, lam, sigma_color, iterations,
              _stream())
    return (out[0], out[1]) if with_weight else out[0]


# ------------------------------------------------------------------------------------ disparity splat
# DESIGN.md section 21.  Forward only, one kernel: the left disparity forward-warped into the right view, nearest surface winning.
def disparity_splat_max_width():
    """The widest map disparity_splat takes (a size query of the library: no GPU needed)."""
    return int(_lib.query("ecm_disp_splat_max_width"))


@torch.no_grad()
def disparity_splat(disp, with_source=False):
    """The left-view disparity disp ([B,H,W] or [B,1,H,W], pixels) forward-warped into the right view, as a [B,H,W] plane: pixel x
    with a finite d and x - d inside [0, W-1] lands on floor(x - d) and, where x - d is not integral, on the column after it -- the
    columns lr_check reads for that pixel -- and per right-view column the largest disparity wins (the nearest surface; among
    equal disparities the larger source column; -0.0 loses to +0.0).  The winner's disparity is copied bit for bit; a column on
    which nothing landed (a hole) is 0.  with_source=True returns (right, src), src int32: the winner's left column, -1 for a hole.
    Fed to lr_check(disp, right, mirrored=False) it marks the occlusions that disp's own geometry implies, from one inference:
    every in-view pixel reads only columns it wrote to, so r >= d, error = r - d and kind 2 never occurs.  Integer maxima only:
    bit-reproducible."""
    disp = _disp_plane("disparity_splat", disp, "want a non-empty [B,H,W] or [B,1,H,W]")
    B, H, W = disp.shape
    d = _c(disp.detach())
    right = torch.empty(B, H, W, device=d.device, dtype=d.dtype)
    src = torch.empty(B, H, W, device=d.device, dtype=torch.int32) if with_source else None
    # W beyond disparity_splat_max_width() is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecm_disp_splat_fwd", _p(d), _p(right), _p(src), B, H, W, _stream())
    return (right, src) if with_source else right


# ------------------------------------------------------------------------------------ disparity reprojection
# DESIGN.md section 23; include/ecm_geometry.h.  Forward only: [X Y Z W]^T = Q [x y d 1]^T in fp64 on the device, the point
# (X/W, Y/W, Z/W) rounded once to fp32 -- OpenCV's reprojectImageTo3D -- as a dense map and as a packed cloud.
REPROJECT_MAX_ATTRIBUTES = 4


def q_matrix(focal, baseline, cx, cy, cx_right=None, x0=0, y0=0):
    """The 4x4 disparity-to-depth matrix of a rectified pair, in stereoRectify's form with a POSITIVE baseline, as a float64 CPU
    tensor: rows [1,0,0,-(cx-x0)], [0,1,0,-(cy-y0)], [0,0,0,f], [0,0,1/b,-(cx-cx_right)/b], so that Z = f b / (d - (cx - cx_right)),
    X = (x + x0 - cx) Z / f and Y = (y + y0 - cy) Z / f.  focal and the principal point (cx, cy; cx_right: the right camera's, None
    for the same) are in pixels of the full frame, baseline in the unit the points come out in; (x0, y0) is the origin of the crop
    that the disparity map covers (what frame_prep was given as crop_x0, crop_y0)."""
    vals = {"focal": focal, "baseline": baseline, "cx": cx, "cy": cy, "cx_right": cx if cx_right is None else cx_right, "x0": x0, "y0": y0}
    for name, v in vals.items():
        _real("q_matrix", name, v)
    if focal <= 0 or baseline <= 0:
        raise ValueError(f"q_matrix: focal {focal!r} and baseline {baseline!r}: both > 0")
    f, b = float(focal), float(baseline)
    return torch.tensor([[1.0, 0.0, 0.0, float(x0) - float(cx)],
                         [0.0, 1.0, 0.0, float(y0) - float(cy)],
                         [0.0, 0.0, 0.0, f],
                         [0.0, 0.0, 1.0 / b, (float(vals["cx_right"]) - float(cx)) / b]], dtype=torch.float64)


def check_reproject_parameters(Q, min_disp=0.0, max_disp=None, n_attributes=0, who="disparity_reproject", name="Q"):
    """(min_disp, max_disp) as the two floats the library takes, after refusing -- before any device work -- a Q that is not a
    floating-point [4,4] or [B,4,4] tensor or, where it lies on the CPU, has a non-finite entry (a Q already on the device is not
    read back: its entries are the caller's), a min_disp that is not a finite fp32 value, a max_disp below it, and more than four
    attribute planes.  max_disp None or beyond the largest float is that float: a usable disparity is finite.  name: what the
    messages call the matrix (disparity_warp's is M)."""
    if not isinstance(Q, torch.Tensor) or not Q.is_floating_point() or Q.dim() not in (2, 3) or tuple(Q.shape[-2:]) != (4, 4) \
            or Q.shape[0] < 1:
        what = f"{tuple(Q.shape)} {Q.dtype}" if isinstance(Q, torch.Tensor) else type(Q).__name__
        raise ValueError(f"{who}: {name} {what}: a floating-point [4,4] or [B,4,4] tensor")
    if not Q.is_cuda and not bool(torch.isfinite(Q).all()):
        raise ValueError(f"{who}: {name} has a non-finite entry")
    _real(who, "min_disp", min_disp, fp32=True)
    if max_disp is None:
        max_disp = _FLT_MAX
    if isinstance(max_disp, bool) or not isinstance(max_disp, numbers.Real) or not max_disp >= min_disp:
        raise ValueError(f"{who}: max_disp {max_disp!r}: None or a number >= min_disp ({min_disp!r})")
    if not 0 <= n_attributes <= REPROJECT_MAX_ATTRIBUTES:
        raise ValueError(f"{who}: {n_attributes} attribute planes: at most {REPROJECT_MAX_ATTRIBUTES}")
    return float(min_disp), min(float(max_disp), _FLT_MAX)


def _reproject_operands(who, disp, Q, attributes, valid, min_disp, max_disp, name="Q"):
    """Every refusal of the two ops (and of disparity_warp, whose matrix is called M: `name`), then the operands:
    (d, v, q, per_image, a, lo, hi); q the float64 device copy of Q."""
    if attributes is not None:
        _need(isinstance(attributes, torch.Tensor) and attributes.dim() == 4,
              lambda: f"{who}: attributes {tuple(getattr(attributes, 'shape', ()))}: want [B,C,H,W]")
    lo, hi = check_reproject_parameters(Q, min_disp, max_disp, 0 if attributes is None else attributes.shape[1], who, name)
    d, v = _filter_planes(who, disp, valid)
    B, H, W = d.shape
    if Q.dim() == 3 and Q.shape[0] != B:
        raise ValueError(f"{who}: {name} {tuple(Q.shape)} against disp {tuple(d.shape)}: one matrix, or one per image")
    a = None
    if attributes is not None and attributes.shape[1] > 0:
        _chk(attributes)
        _need(attributes.shape[0] == B and tuple(attributes.shape[2:]) == (H, W),
              lambda: f"{who}: attributes {tuple(attributes.shape)} against disp {tuple(d.shape)}: want [B,C,H,W]")
        a = _c(attributes.detach())
    q = Q.detach().to(device=d.device, dtype=torch.float64).contiguous()
    return d, v, q, int(Q.dim() == 3), a, lo, hi


@torch.no_grad()
def disparity_reproject(disp, Q, valid=None, min_disp=0.0, max_disp=None, with_mask=False):
    """The 3-D point of every pixel of disp ([B,H,W] or [B,1,H,W], pixels) as xyz [B,3,H,W]: [X Y Z W]^T = Q [x y d 1]^T in fp64
    and (X/W, Y/W, Z/W), each rounded once to fp32 (OpenCV's reprojectImageTo3D; Q: [4,4] or [B,4,4], on the CPU or the device,
    any float dtype, converted once to float64 on the device; ops.q_matrix builds one).  A pixel is usable where d is finite,
    valid != 0 (bool or uint8 of disp's shape; None: all ones), min_disp < d <= max_disp (fp32; None: no upper bound) and W is
    finite and non-zero; every other pixel is +0.0 in all three planes.  with_mask=True returns (xyz, mask), mask bool [B,H,W].
    One launch, no atomics: bit-reproducible.  The defaults say nothing about EPE or D1, and Q's sign conventions are the
    caller's."""
    d, v, q, per_image, _, lo, hi = _reproject_operands("disparity_reproject", disp, Q, None, valid, min_disp, max_disp)
    B, H, W = d.shape
    xyz = torch.empty(B, 3, H, W, device=d.device, dtype=d.dtype)
    mask = torch.empty(B, H, W, device=d.device, dtype=torch.uint8) if with_mask else None
    # B * H * W >= 2^31 is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecmg_reproject_fwd", _p(d), _p(v), _p(q), per_image, _p(xyz), _p(mask), B, H, W, lo, hi, _stream())
    return (xyz, mask.view(torch.bool)) if with_mask else xyz


def point_cloud_tile():
    """The pixels of one compaction tile of point_cloud (a size query of the library: no GPU needed)."""
    return int(_lib.query("ecmg_point_cloud_tile"))


@torch.no_grad()
def point_cloud(disp, Q, attributes=None, valid=None, min_disp=0.0, max_disp=None, with_dense=False):
    """The usable pixels of disparity_reproject as a packed cloud: (points, offsets), points [N, 3 + C] fp32 -- a row is
    (X/W, Y/W, Z/W) and the pixel's values in the C planes of attributes ([B,C,H,W] fp32, C in 0..4; e.g. the left image for
    XYZRGB), bit for bit -- and offsets [B + 1] int64: image b's points are rows offsets[b]..offsets[b+1], in row-major pixel
    order.  The order is the pixel order whatever the scheduling (three launches, no atomics, no workgroup waits for another):
    bit-reproducible, and an image's rows do not depend on the rest of the batch.  The op allocates the worst case (B*H*W rows),
    reads offsets[B] on the host -- its one synchronisation -- and returns the [:N] view; N = 0 gives an empty [0, 3 + C]
    tensor.  with_dense=True returns (points, offsets, xyz, mask): disparity_reproject's outputs, bit for bit, written in the
    same pass.  disp, Q, valid, min_disp and max_disp as in disparity_reproject."""
    d, v, q, per_image, a, lo, hi = _reproject_operands("point_cloud", disp, Q, attributes, valid, min_disp, max_disp)
    B, H, W = d.shape
    C_ = 0 if a is None else a.shape[1]
    nb = _lib.query("ecmg_point_cloud_scratch_bytes", B, H, W)
    _need(nb > 0, lambda: f"point_cloud: disp {tuple(d.shape)}: more pixels than the kernels are built for (B*H*W < 2^31)")
    points = torch.empty(B * H * W, 3 + C_, device=d.device, dtype=d.dtype)
    offsets = torch.empty(B + 1, device=d.device, dtype=torch.int64)
    xyz = torch.empty(B, 3, H, W, device=d.device, dtype=d.dtype) if with_dense else None
    mask = torch.empty(B, H, W, device=d.device, dtype=torch.uint8) if with_dense else None
    scratch = _scratch(nb, d.device)
    _lib.call("ecmg_point_cloud_fwd", _p(d), _p(v), _p(q), per_image, _p(a), C_, _p(points), _p(offsets), _p(xyz), _p(mask),
              _p(scratch), C.c_longlong(nb), B, H, W, lo, hi, _stream())
    n = int(offsets[B].item())                                         # the one host synchronisation
    points = points[:n]
    return (points, offsets, xyz, mask.view(torch.bool)) if with_dense else (points, offsets)


# ------------------------------------------------------------------------------------ temporal carry: pose warp and fusion
# DESIGN.md section 30; include/ecm_temporal.h.  Forward only: a disparity map carried to the next frame by a known camera motion
# -- one fp64 matrix per image, a z-buffered 2-D scatter -- and a per-pixel Kalman update behind it.
WARP_FOOTPRINTS = ("cover", "nearest")                                 # the `footprint` of ecmt_disparity_warp_fwd: 0, 1


def disparity_warp_max_attributes():
    """The most attribute planes disparity_warp carries (a size query of the library: no GPU needed)."""
    return int(_lib.query("ecmt_disparity_warp_max_attributes"))


def _pose(who, name, t):
    """t, a float64 CPU [4,4] or [B,4,4] tensor with finite entries, or ValueError."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.is_cuda or t.dim() not in (2, 3) \
            or tuple(t.shape[-2:]) != (4, 4) or t.shape[0] < 1:
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name} {what}: a float64 CPU [4,4] or [B,4,4] tensor")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{who}: {name} has a non-finite entry")
    return t.detach()


def warp_matrix(Q, T, Q_out=None):
    """M = inv(Q_out) @ T @ Q in float64 on the CPU, [4,4] or (where any operand is batched) [B,4,4]: the matrix that
    disparity_warp applies to (x, y, d, 1).  Q and Q_out (None: Q) are the disparity-to-depth matrices of the previous and the
    current frame, as q_matrix / stereo_rectify return them; T takes points of the previous left-camera frame to the current
    one, in the unit of Q's baseline.  Q is projective, so T Q (x, y, d, 1) is the moved point in homogeneous coordinates and
    inv(Q_out) takes it back to a pixel and a disparity: the whole motion is one matrix.  T need not be rigid -- any finite 4x4 is
    applied as it is.  Rigid means T = [[R, t], [0, 1]] with R a rotation (R^T R = I, det R = +1): that is the caller's to
    supply, for a static scene seen from a moving camera the inverse of the camera's own motion.  ValueError, before any device
    work, for an operand that is not a float64 CPU [4,4] or [B,4,4] tensor, disagreeing batch sizes, a non-finite entry or a
    singular Q_out."""
    Q, T = _pose("warp_matrix", "Q", Q), _pose("warp_matrix", "T", T)
    Q_out = Q if Q_out is None else _pose("warp_matrix", "Q_out", Q_out)
    batches = {t.shape[0] for t in (Q, T, Q_out) if t.dim() == 3}
    if len(batches) > 1:
        raise ValueError(f"warp_matrix: Q {tuple(Q.shape)}, T {tuple(T.shape)}, Q_out {tuple(Q_out.shape)}: one batch size")
    inv, info = torch.linalg.inv_ex(Q_out)
    if bool((info != 0).any()) or not bool(torch.isfinite(inv).all()):
        raise ValueError("warp_matrix: Q_out is singular")
    return inv @ T @ Q


def check_warp_parameters(M, min_disp=0.0, max_disp=None, n_attributes=0, footprint="cover", who="disparity_warp"):
    """(min_disp, max_disp, footprint) as the two floats and the int the library takes, after refusing -- before any device work
    -- an M that is not a float64 [4,4] or [B,4,4] tensor or, where it lies on the CPU, has a non-finite entry, a min_disp that
    is not a finite fp32 value, a max_disp below it, more than disparity_warp's four attribute planes and a footprint other than
    "cover" or "nearest"."""
    if footprint not in WARP_FOOTPRINTS:
        raise ValueError(f"{who}: footprint {footprint!r}: one of {WARP_FOOTPRINTS}")
    if isinstance(M, torch.Tensor) and M.dtype != torch.float64:
        raise ValueError(f"{who}: M is {M.dtype}: want float64 (ops.warp_matrix builds one)")
    lo, hi = check_reproject_parameters(M, min_disp, max_disp, n_attributes, who, "M")
    return lo, hi, WARP_FOOTPRINTS.index(footprint)


@torch.no_grad()
def disparity_warp(disp, M, valid=None, attributes=None, min_disp=0.0, max_disp=None, footprint="cover", with_source=False):
    """disp ([B,H,W] or [B,1,H,W], pixels) carried into another frame by M (float64 [4,4] or [B,4,4], on the CPU or the device;
    ops.warp_matrix builds one), with a z-buffer, as out [B,1,H,W].  A pixel is usable by disparity_reproject's rule (d finite,
    valid != 0, min_disp < d <= max_disp, the fourth row's w finite and non-zero).  [a b c w]^T = M [x y d 1]^T in fp64 in
    disparity_reproject's order; the pixel is a candidate where u = a/w, v = b/w and dn = (float)(c/w) are finite, dn > 0,
    0 <= u <= W-1 and 0 <= v <= H-1.  footprint "cover": it lands on (floor u, floor v), on the next column too iff u is not
    integral, on the next row too iff v is not -- up to four sites, so that a surface that the motion magnifies (by less than
    two) leaves no holes, at the price of foreground edges up to one pixel thicker (as disparity_splat's); "nearest": on the
    one site (floor(u + 0.5), floor(v + 0.5)).  Per site the largest dn wins (the nearest surface), among equals the larger
    source index y * W + x.  out is the winner's dn bit for bit and +0.0 for a hole.  attributes ([B,C,H,W] fp32, C <= 4): also
    returns attrs_out [B,C,H,W], the planes at the winner's source pixel bit for bit, +0.0 for a hole.  with_source=True: also
    src [B,1,H,W] int32, the winner's index, -1 for a hole.  Returns out, (out, src), (out, attrs_out) or (out, attrs_out, src).
    Integer maxima only: bit-reproducible, and an image does not depend on the rest of the batch.  A static-scene model: what
    moved on its own is warped as if it had not."""
    if attributes is not None:
        _need(isinstance(attributes, torch.Tensor) and attributes.dim() == 4,
              lambda: f"disparity_warp: attributes {tuple(getattr(attributes, 'shape', ()))}: want [B,C,H,W]")
    _, _, fp = check_warp_parameters(M, min_disp, max_disp, 0 if attributes is None else attributes.shape[1], footprint)
    d, v, m, per_image, a, lo, hi = _reproject_operands("disparity_warp", disp, M, attributes, valid, min_disp, max_disp, "M")
    B, H, W = d.shape
    C_ = 0 if a is None else a.shape[1]
    nb = _lib.query("ecmt_disparity_warp_scratch_bytes", B, H, W)
    _need(nb > 0, lambda: f"disparity_warp: disp {tuple(d.shape)}: more pixels than the kernels are built for (H*W < 2^31)")
    out = torch.empty(B, 1, H, W, device=d.device, dtype=d.dtype)
    src = torch.empty(B, 1, H, W, device=d.device, dtype=torch.int32) if with_source else None
    attrs_out = torch.empty(B, C_, H, W, device=d.device, dtype=d.dtype) if attributes is not None else None
    scratch = _scratch(nb, d.device)
    _lib.call("ecmt_disparity_warp_fwd", _p(d), _p(v), _p(m), per_image, _p(a), C_, _p(out), _p(src),
              _p(attrs_out if C_ else None), _p(scratch), C.c_longlong(nb), B, H, W, lo, hi, fp, _stream())
    res = (out,) + ((attrs_out,) if attributes is not None else ()) + ((src,) if with_source else ())
    return res if len(res) > 1 else out


def check_fuse_parameters(gate=3.0, process_noise=0.0, coast=True, who="disparity_fuse"):
    """(gate, process_noise, coast) as two floats and an int: both numbers finite fp32 values >= 0, coast a bool."""
    if not isinstance(coast, bool):
        raise ValueError(f"{who}: coast {coast!r}: True or False")
    return _real(who, "gate", gate, ">= 0", fp32=True), _real(who, "process_noise", process_noise, ">= 0", fp32=True), int(coast)


@torch.no_grad()
def disparity_fuse(disp, var, prev, prev_var, prev_age=None, prev_source=None, gate=3.0, process_noise=0.0, coast=True):
    """(fused, fused_var, age), each [B,1,H,W] (age int32): the per-pixel scalar Kalman update of a state carried into this frame
    (prev, prev_var, prev_age: disparity_warp's outputs) with the frame's own estimate (disp and its variance var, e.g.
    predict's std squared).  A measurement exists where disp and var are finite and > 0, a prediction where prev > 0 and prev_var
    is finite and > 0.  The predicted variance s = prev_var + process_noise; with prev_source (the disparity the winner had
    before the warp, carried as an attribute) s = prev_var * r^4 + process_noise, r = prev / prev_source -- the first-order
    propagation of a disparity's variance for a motion along the optical axis, and only that: a rotation or a sideways motion
    changes the disparity by an amount that does not scale it.  Both exist and (disp - prev)^2 <= gate^2 (s + var):
    K = s / (s + var), fused = prev + K (disp - prev), fused_var = (1 - K) s, age = prev_age + 1.  Both exist and the gate fails
    (a moving object, a disocclusion), or only a measurement: (disp, var, 1).  Only a prediction: (prev, s, prev_age) with
    coast, else zeros.  Neither: zeros.  prev_age: int32, None for all zeros.  One launch, fp32 in a fixed order:
    bit-reproducible.  Every plane [B,H,W] or [B,1,H,W] of disp's shape."""
    who = "disparity_fuse"
    gate, process_noise, coast = check_fuse_parameters(gate, process_noise, coast)          # before any device work
    d = _disp_plane(who, disp)
    f32 = ((torch.float32,), "fp32")
    planes = [_c(d.detach())] + [_c(_plane_like(who, n, t, d, *f32)) for n, t in (("var", var), ("prev", prev), ("prev_var", prev_var))]
    age_in = None if prev_age is None else _c(_plane_like(who, "prev_age", prev_age, d, (torch.int32,), "int32"))
    source = None if prev_source is None else _c(_plane_like(who, "prev_source", prev_source, d, *f32))
    B, H, W = d.shape
    fused, fused_var = (torch.empty(B, 1, H, W, device=d.device, dtype=d.dtype) for _ in range(2))
    age = torch.empty(B, 1, H, W, device=d.device, dtype=torch.int32)
    _lib.call("ecmt_disparity_fuse_fwd", *(_p(t) for t in planes), _p(age_in), _p(source), _p(fused), _p(fused_var), _p(age),
              C.c_longlong(B * H * W), gate, process_noise, coast, _stream())
    return fused, fused_var, age


# ------------------------------------------------------------------------------------ camera motion: dense disparity alignment
# DESIGN.md section 31; include/ecm_motion.h.  Forward only: the rigid motion that maps one disparity map onto the next, by
# Gauss-Newton on the residual in disparity space.  The device forms the 27 sums of the normal equations in one call; the 6x6
# solve and the pose update are fp64 on the host.
_SE3_SERIES = 0.1            # below this angle the coefficients are their Taylor series (truncated below 1e-17 relative)


def _twists(who, name, t, last):
    """t, a float64 CPU tensor [last...] or [B, last...] with finite entries, as ([B, last...], was it batched), or ValueError."""
    n = len(last)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.is_cuda or t.dim() not in (n, n + 1) \
            or tuple(t.shape[-n:]) != last or t.shape[0] < 1:
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name} {what}: a float64 CPU tensor {list(last)} or [B, {', '.join(map(str, last))}]")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{who}: {name} has a non-finite entry")
    t = t.detach()
    return (t, True) if t.dim() == n + 1 else (t.unsqueeze(0), False)


def _hat(w):
    """[B,3] -> the skew matrices [B,3,3]: hat(w) x = w cross x."""
    K = torch.zeros(w.shape[0], 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return K


def se3_exp(xi):
    """The rigid motion exp(xi^) of a twist xi = (nu, omega), float64 on the CPU, [6] -> [4,4] or [B,6] -> [B,4,4]:
    R = I + a K + b K^2 and t = (I + b K + c K^2) nu with K = hat(omega), th = |omega|, a = sin th / th, b = (1 - cos th) / th^2,
    c = (th - sin th) / th^3.  Below th = 0.1 the three are their Taylor series, so exp(0) is the identity exactly."""
    xi, batched = _twists("se3_exp", "xi", xi, (6,))
    nu, om = xi[:, :3], xi[:, 3:]
    t2 = (om * om).sum(1)
    th = torch.sqrt(t2)
    small = th < _SE3_SERIES
    ts = torch.where(small, torch.ones_like(th), th)
    half = torch.sin(ts / 2.0) / (ts / 2.0)
    a = torch.where(small, 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110)))), torch.sin(ts) / ts)
    b = torch.where(small, 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56 * (1 - t2 / 90 * (1 - t2 / 132))))), 0.5 * half * half)
    c = torch.where(small, (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110 * (1 - t2 / 156))))) / 6,
                    (ts - torch.sin(ts)) / (ts * ts * ts))
    K = _hat(om)
    K2 = K @ K
    eye = torch.eye(3, dtype=torch.float64)
    T = torch.zeros(xi.shape[0], 4, 4, dtype=torch.float64)
    T[:, :3, :3] = eye + a[:, None, None] * K + b[:, None, None] * K2
    T[:, :3, 3] = ((eye + b[:, None, None] * K + c[:, None, None] * K2) @ nu[:, :, None])[:, :, 0]
    T[:, 3, 3] = 1.0
    return T if batched else T[0]


def se3_log(T):
    """The twist xi = (nu, omega) with exp(xi^) = T, float64 on the CPU, [4,4] -> [6] or [B,4,4] -> [B,6]; |omega| in [0, pi].  T's
    rotation block is taken as orthonormal and its bottom row is not read.  nu = (I - K / 2 + d K^2) t with K = hat(omega),
    d = (1 - a / (2 b)) / th^2 in se3_exp's a and b, its Taylor series below th = 0.1.  se3_log(se3_exp(xi)) is xi to rounding
    for |omega| < pi."""
    T, batched = _twists("se3_log", "T", T, (4, 4))
    om = torch.stack([_rotation_vector(R) for R in T[:, :3, :3]])
    t2 = (om * om).sum(1)
    th = torch.sqrt(t2)
    small = th < _SE3_SERIES
    ts = torch.where(small, torch.ones_like(th), th)
    half = torch.sin(ts / 2.0) / (ts / 2.0)
    a, b = torch.sin(ts) / ts, 0.5 * half * half
    d = torch.where(small, 1.0 / 12 + t2 / 720 + t2 * t2 / 30240 + t2 * t2 * t2 / 1209600, (1 - a / (2 * b)) / (ts * ts))
    K = _hat(om)
    Vinv = torch.eye(3, dtype=torch.float64) - 0.5 * K + d[:, None, None] * (K @ K)
    xi = torch.cat([(Vinv @ T[:, :3, 3:4])[:, :, 0], om], 1)
    return xi if batched else xi[0]


ALIGN_SUMS = 32                                                        # doubles per image of motion_normal


def align_sums():
    """The doubles per image that motion_normal returns (a size query of the library: no GPU needed); ALIGN_SUMS restates it."""
    return int(_lib.query("ecmm_align_sums"))


def check_align_parameters(step=1, min_disp=0.0, max_disp=None, tap_range=1.0, max_residual=3.0, cauchy=1.0, who="motion_normal"):
    """(step, min_disp, max_disp, tap_range, max_residual, cauchy) as the int and the five floats the library takes: step an
    integer >= 1, min_disp a finite fp32 value, max_disp None (no upper bound) or a number >= min_disp, the other three finite
    fp32 values > 0.  ValueError otherwise, before any device work."""
    step = _integer(who, "step", step, 1, 2 ** 31 - 1)
    lo, hi = check_reproject_parameters(torch.eye(4, dtype=torch.float64), min_disp, max_disp, 0, who)
    return (step, lo, hi) + tuple(_real(who, n, v, "> 0", fp32=True)
                                  for n, v in (("tap_range", tap_range), ("max_residual", max_residual), ("cauchy", cauchy)))


def _align_matrices(who, Q, T, Q_out):
    """(Q, inv(Q_out), T) after their refusals: Q and Q_out float64 CPU [4,4], T float64 CPU [4,4] or [B,4,4], Q_out regular."""
    Q, T = _pose(who, "Q", Q), _pose(who, "T", T)
    Q_out = Q if Q_out is None else _pose(who, "Q_out", Q_out)
    if Q.dim() != 2 or Q_out.dim() != 2:
        raise ValueError(f"{who}: Q {tuple(Q.shape)}, Q_out {tuple(Q_out.shape)}: one [4,4] matrix each for the batch")
    inv, info = torch.linalg.inv_ex(Q_out)
    if bool((info != 0).any()) or not bool(torch.isfinite(inv).all()):
        raise ValueError(f"{who}: Q_out is singular")
    return Q, inv, T


@torch.no_grad()
def motion_normal(disp0, disp1, Q, T, valid0=None, valid1=None, weight=None, Q_out=None, step=1, min_disp=0.0, max_disp=None,
                  tap_range=1.0, max_residual=3.0, cauchy=1.0, with_residual=False):
    """The normal equations of one Gauss-Newton step of the alignment of disp0 (the source: the previous frame or a carried
    state) to disp1 (the target: this frame), both [B,H,W] or [B,1,H,W] fp32 with H, W >= 2, under the motion estimate T (float64
    CPU [4,4] or [B,4,4]; it takes points of the source frame to the target frame): sums [B,32] float64 on the device, one kernel
    call.  Per source pixel of the lattice x % step == 0, y % step == 0 that is usable by disparity_reproject's rule (valid0,
    min_disp, max_disp, Q) and whose weight ([B,H,W] fp32, the inverse variance of the residual; None: 1) is finite and > 0: the
    point is moved by T, projected by inv(Q_out) (Q_out None: Q; both float64 CPU [4,4]) to (u, v, dn); disp1 is sampled
    bilinearly at (u, v) where its four taps are usable (valid1) and within tap_range of one another; the residual is
    r = sample - dn, dropped beyond max_residual; J is its derivative for a left-multiplied twist; the Cauchy weight is
    1 / (1 + weight r^2 / cauchy^2).  sums[b]: [0..20] the upper triangle of sum a J^T J, [21..26] sum a J^T r, [27] sum a r^2,
    [28] sum a, [29] the pixels used, [30] the candidates (projected into view), [31] 0 -- include/ecm_motion.h states every
    operation.  with_residual=True returns (sums, residual), residual [B,1,H,W] fp32: r at the used source pixels, NaN elsewhere.
    No atomics, a fixed order of additions: bit-reproducible, and an image's sums do not depend on the rest of the batch."""
    who = "motion_normal"
    step, lo, hi, tap_range, max_residual, cauchy = check_align_parameters(step, min_disp, max_disp, tap_range, max_residual, cauchy)
    Q, Qinv, T = _align_matrices(who, Q, T, Q_out)
    d0, v0 = _filter_planes(who, disp0, valid0)
    B, H, W = d0.shape
    _need(H >= 2 and W >= 2, lambda: f"{who}: disp0 {tuple(d0.shape)}: H and W at least 2 (the target is sampled bilinearly)")
    if T.dim() == 3 and T.shape[0] != B:
        raise ValueError(f"{who}: T {tuple(T.shape)} against disp0 {tuple(d0.shape)}: one matrix, or one per image")
    f32 = ((torch.float32,), "fp32")
    d1 = _c(_plane_like(who, "disp1", disp1, d0, *f32))
    v1 = None if valid1 is None else _mask_plane(who, valid1, d0)
    w0 = None if weight is None else _c(_plane_like(who, "weight", weight, d0, *f32))
    nb = _lib.query("ecmm_align_scratch_bytes", B, H, W, step)
    _need(nb > 0, lambda: f"{who}: disp0 {tuple(d0.shape)}: more pixels than the kernels are built for (H*W < 2^31)")
    mats = torch.cat([Q.reshape(-1), Qinv.reshape(-1), T.reshape(-1)]).to(d0.device)          # one host-to-device copy
    sums = torch.empty(B, ALIGN_SUMS, device=d0.device, dtype=torch.float64)
    residual = torch.empty(B, 1, H, W, device=d0.device, dtype=d0.dtype) if with_residual else None
    scratch = _scratch(nb, d0.device)
    at = mats.data_ptr()
    _lib.call("ecmm_align_normal_fwd", _p(d0), _p(v0), _p(w0), _p(d1), _p(v1), C.c_void_p(at), C.c_void_p(at + 128),
              C.c_void_p(at + 256), int(T.dim() == 3), _p(sums), _p(residual), _p(scratch), C.c_longlong(nb), B, H, W, step, lo, hi,
              tap_range, max_residual, cauchy, _stream())
    return (sums, residual) if with_residual else sums


# What motion_estimate returns.  T [B,4,4] float64 on the CPU, in the form DisparityTracker takes as `motion`; per image:
# converged (bool), iterations (int64: the steps taken), used and candidates (int64: the pixels of the last sums), rms
# (sqrt(sums[27] / sums[28]) of the last sums; NaN where nothing was used) and information [B,6,6], the last J^T J (undamped).
MotionEstimate = collections.namedtuple("MotionEstimate", "T converged iterations used candidates rms information")


def unpack_align_sums(sums):
    """(H [B,6,6], g [B,6]) of sums [B,32]: the symmetric J^T J from its upper triangle, and J^T r."""
    iu = torch.triu_indices(6, 6)
    H = torch.zeros(sums.shape[0], 6, 6, dtype=sums.dtype)
    H[:, iu[0], iu[1]] = sums[:, :21]
    H[:, iu[1], iu[0]] = sums[:, :21]
    return H, sums[:, 21:27]


def check_estimate_parameters(iterations=10, damping=1e-6, tolerance=1e-7, min_pixels=64, who="motion_estimate"):
    """(iterations, damping, tolerance, min_pixels): integers >= 1 and finite numbers >= 0, or ValueError."""
    return (_integer(who, "iterations", iterations, 1), _real(who, "damping", damping, ">= 0"),
            _real(who, "tolerance", tolerance, ">= 0"), _integer(who, "min_pixels", min_pixels, 1))


def motion_estimate(disp0, disp1, Q, init=None, valid0=None, valid1=None, weight=None, Q_out=None, step=1, min_disp=0.0,
                    max_disp=None, tap_range=1.0, max_residual=3.0, cauchy=1.0, iterations=10, damping=1e-6, tolerance=1e-7,
                    min_pixels=64, normal=None):
    """The rigid motion T that maps the disparity surface of disp0 onto disp1 (motion_normal's operands), by at most `iterations`
    Gauss-Newton steps from init (float64 CPU [4,4] or [B,4,4]; None: the identity): per step one motion_normal call, one
    device-to-host copy of its [B,32] sums, the solve of (H + damping diag(H)) xi = -g in fp64 on the host, and
    T <- se3_exp(xi) T.  An image stops, converged, once |xi| < tolerance.  An image with fewer than min_pixels used pixels or a
    system that cannot be solved stops with its init as T and converged False: never a NaN pose.  Returns a MotionEstimate.
    normal: a callable T [B,4,4] -> sums [B,32] that replaces motion_normal (disp0 then only gives B, and nothing is launched):
    the loop itself runs on the host.  A static-scene estimator without a pyramid: see DESIGN.md section 31 for what it cannot
    do; every default is untested for quality."""
    who = "motion_estimate"
    iterations, damping, tolerance, min_pixels = check_estimate_parameters(iterations, damping, tolerance, min_pixels)
    check_align_parameters(step, min_disp, max_disp, tap_range, max_residual, cauchy, who)
    B = disp0.shape[0]
    init = torch.eye(4, dtype=torch.float64) if init is None else _pose(who, "init", init)
    if init.dim() == 3 and init.shape[0] != B:
        raise ValueError(f"{who}: init {tuple(init.shape)} against disp0 {tuple(disp0.shape)}: one matrix, or one per image")
    init = (init.expand(B, 4, 4) if init.dim() == 2 else init).clone()
    if normal is None:
        def normal(T):
            return motion_normal(disp0, disp1, Q, T, valid0, valid1, weight, Q_out, step, min_disp, max_disp, tap_range,
                                 max_residual, cauchy)
    T = init.clone()
    active = torch.ones(B, dtype=torch.bool)
    converged = torch.zeros(B, dtype=torch.bool)
    steps = torch.zeros(B, dtype=torch.int64)
    last = torch.zeros(B, ALIGN_SUMS, dtype=torch.float64)
    for _ in range(iterations):
        sums = normal(T).detach().to(device="cpu", dtype=torch.float64)                      # the one device-to-host copy
        last[active] = sums[active]
        H, g = unpack_align_sums(sums)
        A = H + damping * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        xi, info = torch.linalg.solve_ex(A, -g.unsqueeze(2))
        xi = xi[:, :, 0]
        solved = (info == 0) & torch.isfinite(xi).all(1) & torch.isfinite(sums).all(1) & (sums[:, 29] >= min_pixels)
        failed = active & ~solved
        T[failed] = init[failed]
        active = active & solved
        if not bool(active.any()):
            break
        T[active] = se3_exp(xi[active]) @ T[active]
        steps[active] += 1
        done = active & (torch.linalg.vector_norm(xi, dim=1) < tolerance)
        converged |= done
        active = active & ~done
        if not bool(active.any()):
            break
    H, _ = unpack_align_sums(last)
    rms = torch.sqrt(last[:, 27] / last[:, 28])
    return MotionEstimate(T, converged, steps, last[:, 29].to(torch.int64), last[:, 30].to(torch.int64), rms, H)


# ------------------------------------------------------------------------------------ TSDF volume: integrate and raycast
# DESIGN.md section 32; include/ecm_volume.h.  Forward only: disparity maps with their poses are averaged into a dense grid of
# truncated signed distances, and the grid is raycast back into a disparity map from any pose -- the form motion_estimate takes
# as disp0.

# What volume_matrices returns, float64 on the CPU, [4,4] each or (for a batched T) [V,4,4]: G grid -> (u, v, d) of the view, C
# grid -> camera, R (x, y, d) of the output view -> grid, Rinv its inverse.
VolumeMatrices = collections.namedtuple("VolumeMatrices", "G C R Rinv")


def _origin(who, origin):
    """origin as three floats, or ValueError."""
    if isinstance(origin, torch.Tensor) and origin.dim() == 1 and not origin.is_cuda:
        origin = origin.tolist()
    if not isinstance(origin, (tuple, list)) or len(origin) != 3 or not all(_is_real(v) for v in origin):
        raise ValueError(f"{who}: origin {origin!r}: three finite numbers")
    return [float(v) for v in origin]


def volume_matrices(Q, T, origin, voxel, Q_out=None):
    """The per-view matrices of the volume ops, float64 on the CPU: VolumeMatrices(G, C, R, Rinv).  With S = [[voxel I, origin],
    [0, 1]] (grid point (i, j, k) -> the world point origin + voxel (i, j, k)):  C = T S, grid to camera;  G = inv(Q) C, grid to
    (u, v, d) of the view that is integrated;  R = inv(S) inv(T) Q_out, (x, y, d) of the view that is raycast to grid;
    Rinv = inv(Q_out) C, its inverse.  Q and Q_out (None: Q) are disparity-to-depth matrices as q_matrix / stereo_rectify return
    them, one [4,4] each; T is WORLD TO CAMERA, one [4,4] or [V,4,4], and rigid (the world frame is the left-camera frame of the
    first frame: what StereoOdometry's pose maps from).  ValueError, before any device work: what motion_normal refuses of its
    matrices, a voxel that is not a finite number > 0, an origin that is not three finite numbers, a singular Q, and a T whose
    rotation is not orthonormal (R R^T = I to 1e-6, det +1, as stereo_rectify checks it) or whose bottom row is not (0, 0, 0, 1)."""
    who = "volume_matrices"
    Q, Qinv_out, T = _align_matrices(who, Q, T, Q_out)
    voxel = _real(who, "voxel", voxel, "> 0")
    origin = _origin(who, origin)
    Qinv, info = torch.linalg.inv_ex(Q)
    if bool((info != 0).any()) or not bool(torch.isfinite(Qinv).all()):
        raise ValueError(f"{who}: Q is singular")
    Q_out = Q if Q_out is None else Q_out.detach()
    Tb = T if T.dim() == 3 else T.unsqueeze(0)
    rot, eye = Tb[:, :3, :3], torch.eye(3, dtype=torch.float64)
    if float((rot @ rot.transpose(1, 2) - eye).abs().max()) > 1e-6 or float(torch.linalg.det(rot).min()) < 0 \
            or not torch.equal(Tb[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(Tb.shape[0], 4)):
        raise ValueError(f"{who}: T is not rigid (R R^T = I to 1e-6, det +1, bottom row 0 0 0 1)")
    S = torch.eye(4, dtype=torch.float64)
    S[0, 0] = S[1, 1] = S[2, 2] = voxel
    S[:3, 3] = torch.tensor(origin, dtype=torch.float64)
    Sinv = torch.eye(4, dtype=torch.float64)
    Sinv[0, 0] = Sinv[1, 1] = Sinv[2, 2] = 1.0 / voxel
    Sinv[:3, 3] = -torch.tensor(origin, dtype=torch.float64) / voxel
    Tinv = torch.zeros_like(Tb)                                           # a rigid inverse: [[R^T, -R^T t], [0, 1]]
    Tinv[:, :3, :3] = rot.transpose(1, 2)
    Tinv[:, :3, 3:] = -(rot.transpose(1, 2) @ Tb[:, :3, 3:])
    Tinv[:, 3, 3] = 1.0
    C_ = Tb @ S
    out = VolumeMatrices(Qinv @ C_, C_, Sinv @ Tinv @ Q_out, Qinv_out @ C_)
    return out if T.dim() == 3 else VolumeMatrices(*(m[0] for m in out))


def check_volume_parameters(trunc, max_weight=64.0, min_disp=0.0, max_disp=None, who="volume_integrate"):
    """(trunc, max_weight, min_disp, max_disp) as the four floats the library takes: trunc and max_weight finite fp32 values > 0,
    min_disp a finite fp32 value, max_disp None (no upper bound) or a number >= min_disp.  ValueError otherwise."""
    trunc, max_weight = _real(who, "trunc", trunc, "> 0", fp32=True), _real(who, "max_weight", max_weight, "> 0", fp32=True)
    lo, hi = check_reproject_parameters(torch.eye(4, dtype=torch.float64), min_disp, max_disp, 0, who)
    return trunc, max_weight, lo, hi


def raycast_max_steps():
    """The largest max_steps volume_raycast takes (a query of the library: no GPU needed)."""
    return int(_lib.query("ecmv_raycast_max_steps"))


def check_raycast_parameters(size, near_disp, far_disp, step=0.5, max_steps=None, who="volume_raycast"):
    """((H, W), near_disp, far_disp, step, max_steps) as the library takes them: size two integers >= 1, near_disp > far_disp > 0
    and step > 0 finite fp32 values, max_steps None (the library's limit) or an integer in 1..raycast_max_steps()."""
    H, W = _hw(who, "size", size)
    near_disp, far_disp = _real(who, "near_disp", near_disp, "> 0", fp32=True), _real(who, "far_disp", far_disp, "> 0", fp32=True)
    if not near_disp > far_disp:
        raise ValueError(f"{who}: near_disp {near_disp!r} and far_disp {far_disp!r}: near_disp > far_disp > 0")
    step = _real(who, "step", step, "> 0", fp32=True)
    limit = raycast_max_steps()
    return (H, W), near_disp, far_disp, step, limit if max_steps is None else _integer(who, "max_steps", max_steps, 1, limit)


def _volume_dims(who, dims, least=1):
    if not isinstance(dims, (tuple, list, torch.Size)) or len(dims) != 3 or not all(_is_int(n) and n >= least for n in dims):
        raise ValueError(f"{who}: dims {dims!r}: (nz, ny, nx), three integers >= {least}")
    return tuple(int(n) for n in dims)


def volume_new(dims, device):
    """An empty volume of dims = (nz, ny, nx) on `device`: (tsdf, wsum), fp32 [nz,ny,nx] each, tsdf = 1 and wsum = 0."""
    dims = _volume_dims("volume_new", dims)
    if torch.device(device).type != "cuda":
        raise RuntimeError(_CPU_TENSOR)
    tsdf = torch.empty(dims, dtype=torch.float32, device=device)
    tsdf.fill_(1.0)
    return tsdf, torch.zeros(dims, dtype=torch.float32, device=device)


def _no_grad_operands(who, **ts):
    for name, t in ts.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad: the volume ops are forward only")


def _volume_planes(who, least=1, most_attributes=None, **planes):
    """The planes of a volume, by name, after their refusals: tsdf and wsum [nz,ny,nx], and / or attr [A,nz,ny,nx] (A in
    1..most_attributes, the caller's rule) and asum [nz,ny,nx] of the same shape; each a tensor that does not require grad, fp32 on
    the device, contiguous (they are used in place), every dim >= least, and no two sharing a byte.  Returns (nz, ny, nx)."""
    dims, spans = None, []
    for first, second in (("tsdf", "wsum"), ("attr", "asum")):
        if first not in planes:
            continue
        a, b = planes[first], planes[second]
        for name, t in ((first, a), (second, b)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{who}: {name} {type(t).__name__}: a tensor")
            _no_grad_operands(who, **{name: t})
        _chk(a, b)
        if first == "tsdf":
            _need(a.dim() == 3 and a.shape == b.shape and all(n >= least for n in a.shape),
                  lambda: f"{who}: tsdf {tuple(a.shape)}, wsum {tuple(b.shape)}: one shape [nz,ny,nx], every dim >= {least}")
        else:
            _need(b.dim() == 3 and a.dim() == 4 and a.shape[1:] == b.shape and all(n >= least for n in b.shape) and dims in (None, tuple(b.shape)),
                  lambda: f"{who}: attr {tuple(a.shape)}, asum {tuple(b.shape)}: [A,nz,ny,nx] and [nz,ny,nx]"
                  + (f" of the volume's shape {dims}" if dims is not None else f", every dim >= {least}"))
            _need(1 <= a.shape[0] <= most_attributes, lambda: f"{who}: attr {tuple(a.shape)}: A in 1..{most_attributes}")
        _need(a.is_contiguous() and b.is_contiguous(), lambda: f"{who}: {first} and {second} must be contiguous")
        dims = tuple(int(n) for n in b.shape)
        for name, t in ((first, a), (second, b)):
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
            for other, lo2, hi2 in spans:
                _need(hi <= lo2 or hi2 <= lo, lambda: f"{who}: tsdf and wsum are one tensor" if (other, name, lo2) == ("tsdf", "wsum", lo)
                      else f"{who}: {name} and {other} share memory")
            spans.append((name, lo, hi))
    return dims


def _one_device(who, **ts):
    """Every tensor given (None: not passed) lies on the device of the first: the library takes pointers of one device."""
    first = None
    for name, t in ts.items():
        if t is None:
            continue
        if first is None:
            first = (name, t.device)
        _need(t.device == first[1], lambda: f"{who}: {name} is on {t.device}, {first[0]} on {first[1]}: one device")


def _packed_matrices(device, *ms):
    """float64 CPU matrices as one buffer on `device` (one host-to-device copy) and the address of each in it: (buffer, pointers).
    The caller keeps the buffer until its launch is queued."""
    buffer = torch.cat([m.reshape(-1) for m in ms]).to(device)
    sizes = [m.numel() * m.element_size() for m in ms]
    return buffer, [C.c_void_p(buffer.data_ptr() + sum(sizes[:k])) for k in range(len(ms))]


def _integrate_operands(who, planes, disp, Q, T, origin, voxel, trunc, valid, weight, max_weight, min_disp, max_disp, most_attributes=None,
                        **more):
    """What ops.volume_integrate and color.volume_integrate share up to the library call: parameters and matrices before any
    tensor is looked at, then `planes` (by name, for _volume_planes), disp, valid and weight; `more`: the caller's further operands,
    which must not require grad either.  Returns (d, v, w), the entry's (Q, G, C, m_per_view) behind the buffer that holds them,
    (nx, ny, nz), (V, H, W) and (trunc, max_weight, lo, hi).  _one_device is left to the caller, who has every operand."""
    gates = check_volume_parameters(trunc, max_weight, min_disp, max_disp, who)
    m = volume_matrices(Q, T, origin, voxel)
    _no_grad_operands(who, disp=disp, valid=valid, weight=weight, **more)
    nz, ny, nx = _volume_planes(who, most_attributes=most_attributes, **planes)
    d, v = _filter_planes(who, disp, valid)
    if m.G.dim() == 3 and m.G.shape[0] != d.shape[0]:
        raise ValueError(f"{who}: T {tuple(T.shape)} against disp {tuple(d.shape)}: one matrix, or one per view")
    w = None if weight is None else _c(_plane_like(who, "weight", weight, d, ((torch.float32,)), "fp32"))
    mats, pointers = _packed_matrices(d.device, Q.detach(), m.G, m.C)
    return (d, v, w), (mats, *pointers, int(m.G.dim() == 3)), (nx, ny, nz), tuple(d.shape), gates


def _raycast_operands(who, planes, Q_out, T, origin, voxel, size, near_disp, far_disp, step, max_steps, with_weight, most_attributes=None):
    """What ops.volume_raycast and color.volume_raycast share up to the library call.  Returns the entry's (R, Rinv, m_per_view)
    behind the buffer that holds them, (out, hit) -- hit None without with_weight --, (nx, ny, nz), (B, H, W) and the march."""
    (H, W), *march = check_raycast_parameters(size, near_disp, far_disp, step, max_steps, who)
    m = volume_matrices(Q_out, T, origin, voxel)
    nz, ny, nx = _volume_planes(who, least=2, most_attributes=most_attributes, **planes)
    _one_device(who, **planes)
    B = m.R.shape[0] if m.R.dim() == 3 else 1
    dev = planes["tsdf"].device
    mats, pointers = _packed_matrices(dev, m.R, m.Rinv)
    out = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
    hit = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32) if with_weight else None
    return (mats, *pointers, int(m.R.dim() == 3)), (out, hit), (nx, ny, nz), (B, H, W), march


@torch.no_grad()
def volume_integrate(tsdf, wsum, disp, Q, T, origin, voxel, trunc, valid=None, weight=None, max_weight=64.0, min_disp=0.0,
                     max_disp=None):
    """Integrate the V views disp ([V,H,W] or [V,1,H,W] fp32, pixels) into the volume (tsdf, wsum) of volume_new, IN PLACE, and
    return the pair.  Q (float64 CPU [4,4]) is the views' disparity-to-depth matrix, T (float64 CPU [4,4] or [V,4,4]) their
    world-to-camera poses, origin and voxel place the grid (volume_matrices).  Per voxel, the views in order: the voxel is
    projected into the view and rounded to the nearest pixel; the pixel must be usable by disparity_reproject's rule (valid:
    bool or uint8 of disp's shape; min_disp, max_disp) and its weight ([V,H,W] fp32, e.g. 1 / std^2; None: 1) finite and > 0;
    s = (the pixel's depth) - (the voxel's depth), along the optical axis; a voxel more than trunc behind the surface is left
    alone, and otherwise tsdf <- (tsdf wsum + min(1, s / trunc) w) / (wsum + w), wsum <- min(wsum + w, max_weight).  One launch,
    one thread per voxel, no atomics: bit-reproducible; a voxel no view sees keeps its bits.  include/ecm_volume.h states every
    operation.  A static-scene model; every default is untested for quality."""
    who = "volume_integrate"
    (d, v, w), (held, *mats), dims, views, gates = _integrate_operands(who, dict(tsdf=tsdf, wsum=wsum), disp, Q, T, origin, voxel, trunc, valid,
                                                                    weight, max_weight, min_disp, max_disp)
    _one_device(who, tsdf=tsdf, wsum=wsum, disp=d, valid=v, weight=w)
    _lib.call("ecmv_integrate_fwd", _p(tsdf), _p(wsum), _p(d), _p(v), _p(w), *mats, *dims, *views, *gates, _stream())
    return tsdf, wsum


@torch.no_grad()
def volume_raycast(tsdf, wsum, Q_out, T, origin, voxel, size, near_disp, far_disp, step=0.5, max_steps=None, with_weight=False):
    """The disparity map out [B,1,H,W] fp32 that the volume (tsdf, wsum; every dim >= 2) shows to the B views T (float64 CPU
    [4,4]: B = 1, or [B,4,4]; world to camera) with the disparity-to-depth matrix Q_out and size = (H, W).  Per pixel the ray
    from disparity near_disp to far_disp (near_disp > far_disp > 0) is a straight segment of the grid; it is sampled at
    n = ceil(length / step) equal intervals (step in voxels; a pixel with n > max_steps is a hole; None: the library's limit), a
    sample counts where all eight corners of its cell have wsum > 0, and the first front-face zero crossing of the trilinear
    tsdf between two consecutive samples that count, found by linear interpolation, is mapped back to a disparity; a back-face
    crossing met first ends the ray.  Holes are +0.0.  with_weight=True returns (out, hit_weight), the trilinear wsum at the
    crossing.  One launch, one thread per pixel: bit-reproducible.  include/ecm_volume.h states every operation."""
    (held, *mats), (out, hit), dims, views, march = _raycast_operands("volume_raycast", dict(tsdf=tsdf, wsum=wsum), Q_out, T, origin, voxel, size,
                                                                   near_disp, far_disp, step, max_steps, with_weight)
    _lib.call("ecmv_raycast_fwd", _p(tsdf), _p(wsum), *mats, _p(out), _p(hit), *dims, *views, *march, _stream())
    return (out, hit) if with_weight else out


# ------------------------------------------------------------------------------------ a5-a7 conv / deconv / GN
def _pack_conv(w, flip_transpose=False):
    Co, Ci = w.shape[0], w.shape[1]
    kin, kout = (Co, Ci) if flip_transpose else (Ci, Co)
    n = _lib.query("ecm_conv3d_packed_floats", kin, kout)
    packed = torch.empty(n, device=w.device, dtype=w.dtype)
    _lib.call("ecm_conv3d_pack_weight", _p(w), _p(packed), Co, Ci, int(flip_transpose), _stream())
    return packed


def _pack_deconv(w):
    """w [A,Bc,3,3,3]: ConvTranspose3d weight [Ci,Co,...] (or a Conv3d weight whose stride-2 dgrad is wanted)."""
    A, Bc = w.shape[0], w.shape[1]
    n = _lib.query("ecm_conv3d_packed_floats", A, Bc)
    packed = torch.empty(n, device=w.device, dtype=w.dtype)
    _lib.call("ecm_deconv3d_pack_weight", _p(w), _p(packed), A, Bc, _stream())
    return packed


def _wino_ok(x):
    """Winograd kernels read the patch as pairs of neighbouring columns (rows of at least two elements) and address 32
    channel planes with 32-bit byte offsets (a [D,]H,W plane set of at most 2^24 elements); anything else takes the direct
    kernels."""
    vol = x.shape[-1] * x.shape[-2] * (x.shape[-3] if x.dim() == 5 else 1)
    return WINOGRAD and x.shape[-1] >= 2 and vol * 128 <= 0x80000000


def _wino_pack(w, kd, flip_transpose):
    """w: [Co,Ci,3,3,3] (kd 3) or [Co,Ci,3,3] (kd 1), contiguous."""
    Co, Ci = w.shape[:2]
    kin, kout = (Co, Ci) if flip_transpose else (Ci, Co)

    def build():
        packed = torch.empty(_lib.query("ecm_conv_wino_packed_floats", kin, kout, kd), device=w.device, dtype=w.dtype)
        _lib.call("ecm_conv_wino_pack_weight", _p(w), _p(packed), Co, Ci, kd, int(flip_transpose), _stream())
        return packed
    return _cached_pack(w, ("wT" if flip_transpose else "w") + str(kd), build)


def _wino_pack_both(w, kd):
    """(forward layout, data-gradient layout) from ONE launch: what a training step needs of a layer -- the second one is kept on
    the autograd context for the backward of the same step (`_wino_pack_b`), which otherwise packs it in a dependent 5 us launch
    right in front of the data-gradient kernel (67 such launches per step)."""
    Co, Ci = w.shape[:2]
    nf = _lib.query("ecm_conv_wino_packed_floats", Ci, Co, kd)
    nb = _lib.query("ecm_conv_wino_packed_floats", Co, Ci, kd)
    packed = torch.empty(nf + nb, device=w.device, dtype=w.dtype)
    _lib.call("ecm_conv_wino_pack_weight2", _p(w), _p(packed), Co, Ci, kd, _stream())
    return packed[:nf], (packed[nf:], w._version, w.data_ptr())


def _wino_pack_fwd(ctx, x, w, kd, grad_mode):
    """Forward layout of w; in a pass that will need the data gradient, also the backward layout (stored on ctx).
    `grad_mode`: torch.is_grad_enabled() as the CALLER saw it -- inside autograd.Function.forward grad mode is always off, and
    needs_input_grad reflects the inputs' requires_grad flags even under no_grad, so neither can tell an eval call."""
    ctx.packed_b = None
    if grad_mode and ctx.needs_input_grad[0] and not _FROZEN_DEPTH and not torch.cuda.is_current_stream_capturing():
        pf, ctx.packed_b = _wino_pack_both(w, kd)
        return pf
    return _wino_pack(w, kd, False)


def _wino_pack_b(ctx, w, kd):
    """Data-gradient layout: the one packed in forward if the weight has not been written since, else a fresh one."""
    pb = getattr(ctx, "packed_b", None)
    if pb is not None and pb[1] == w._version and pb[2] == w.data_ptr():
        return pb[0]
    return _wino_pack(w, kd, True)


def _wino_run(x, packed, Co, kd, addend=None):
    """x: [B,Ci,D,H,W] (kd 3; or kd 1 on D independent planes) or [B,Ci,H,W] (kd 1) -> same spatial shape with Co channels."""
    B, Ci = x.shape[:2]
    D, H, W = (x.shape[2:] if x.dim() == 5 else (1,) + tuple(x.shape[2:]))
    y = torch.empty((B, Co) + tuple(x.shape[2:]), device=x.device, dtype=x.dtype)
    if addend is None:
        _lib.call("ecm_conv_wino_fwd", _p(x), _p(packed), _p(y), B, Ci, Co, D, H, W, kd, _stream())
    else:                                     # y = conv(x) + addend in the kernel's epilogue (see _fork_grad)
        if addend.shape != y.shape:
            raise RuntimeError("addend must have the shape of the convolution's output")
        _lib.call("ecm_conv_wino_fwd_add", _p(x), _p(packed), _p(_c(addend)), _p(y), B, Ci, Co, D, H, W, kd, _stream())
    return y


# ---- forks: a tensor consumed by a convolution AND by a skip connection ----------------------------------------------------
# Autograd sums the two gradients with a separate elementwise pass (3 passes over the tensor).  With `fork=True` a
# convolution Function also returns its input (as a view), to be used as the skip operand; its backward then receives the
# skip gradient next to the output gradient and adds it in the epilogue of the data-gradient kernel (Winograd path: one extra
# read instead of read + read + write; other paths: a plain add, i.e. what autograd would have done).
def _fork_out(y, x, fork):
    return (y, x.view_as(x)) if fork else y


def _fork_grad(gx, gskip):
    """data gradient + skip gradient where the kernel could not take the addend"""
    if gskip is None:
        return gx
    return gskip if gx is None else gx + gskip


class Fork(torch.autograd.Function):
    """x -> n views of x, one per consumer; backward adds the consumers' gradients in ONE pass (ecm_sum_n: n reads + 1 write)
    instead of autograd's n-1 binary adds of 3 passes each."""

    @staticmethod
    def forward(ctx, x, n):
        _chk(x)                                # backward hands the gradients' addresses to ecm_sum_n as fp32
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [_c(g) for g in grads if g is not None]
        if not gs:
            return None, None
        while len(gs) > 1:
            take, gs = gs[:4], gs[4:]
            if len(take) == 1:
                gs.append(take[0])
                continue
            out = torch.empty_like(take[0])
            take = take + [None] * (4 - len(take))
            _lib.call("ecm_sum_n", _p(take[0]), _p(take[1]), _p(take[2]), _p(take[3]), _p(out), C.c_longlong(out.numel()),
                      _stream())
            gs.insert(0, out)
        return gs[0], None


class ForkHead(torch.autograd.Function):
    """x -> (alias of x, x[:n]): one consumer of the whole batch and one of its first n samples (the encoder's full-resolution
    map: the next encoder layer takes both images, the ECM weights only the left ones, cmfsm.py:657-664).  Autograd's own
    route for that is a zero-filled full-size tensor, a copy of the slice gradient into it and a full-size add (2.8 GB of
    traffic at batch 4); here the full gradient is copied once and the slice gradient added into the copy's first n samples.
    The incoming gradient itself is never written: autograd does not promise that a node owns it (a tensor hook,
    `retain_grad`, a producer that returns one tensor for two inputs, or a `retain_graph` replay may hold the same object).
    Where the consumer of the whole batch is a GroupNorm (cmfsm's encoder) the fork lives inside that node instead
    (GroupNormAct `head`), which adds into its own fresh output with no copy at all."""

    @staticmethod
    def forward(ctx, x, n):
        _chk(x)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return x.view_as(x), x[:n]

    @staticmethod
    def backward(ctx, g_full, g_head):
        if g_head is None:
            return g_full, None
        if g_full is None:
            raise RuntimeError("ForkHead: the full-batch consumer produced no gradient")   # not a configuration of this model
        out = g_full.clone(memory_format=torch.contiguous_format)
        out[:ctx.n].add_(g_head)
        return out, None


def fork_head(x, n):
    """(alias of x, x[:n]) with the slice's gradient folded into the full gradient in place (see ForkHead)."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return x, x[:n]
    return ForkHead.apply(x, int(n))


def fork(x, n):
    """n aliases of x for n consumers whose gradients are then summed by one kernel (see Fork)."""
    if n <= 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * n
    return Fork.apply(x, int(n))


def _conv_fwd(x, packed, Co, stride):
    B, Ci, D, H, W = x.shape
    Do, Ho, Wo = (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(B, Co, Do, Ho, Wo, device=x.device, dtype=x.dtype)
    _lib.call("ecm_conv3d_k3_fwd", _p(x), _p(packed), _p(y), B, Ci, Co, D, H, W, stride, _stream())
    return y


def _deconv_fwd(x, packed, Co, out_dhw):
    B, Ci, D, H, W = x.shape
    Do, Ho, Wo = out_dhw
    y = torch.empty(B, Co, Do, Ho, Wo, device=x.device, dtype=x.dtype)
    _lib.call("ecm_deconv3d_k3s2_fwd", _p(x), _p(packed), _p(y), B, Ci, Co, D, H, W, Do, Ho, Wo, _stream())
    return y


def enable_wgrad_overlap(on=True):
    """Called by a harness that guarantees a join (join_side_streams) before any weight gradient is read; returns the
    previous setting.  The environment's ECM_WGRAD_OVERLAP=0 wins."""
    global WGRAD_OVERLAP
    prev = WGRAD_OVERLAP
    WGRAD_OVERLAP = bool(on) and _WGRAD_ENV != "0"
    return prev


_SIDE = {}     # device index -> [side stream, join queued for the running backward pass, weights seen since the join, event behind the last join]


def pace_side_streams():
    """Block the HOST until the weight gradients of the previous backward pass have finished on the device (returns at once
    when there were none, or during stream capture).  Bounds the caching allocator's pending side-stream blocks to one pass."""
    if not _WGRAD_PACE or not _SIDE:
        return
    for dev, st in list(_SIDE.items()):
        ev = st[3]
        if ev is not None and not torch.cuda.is_current_stream_capturing():
            ev.synchronize()


def join_side_streams():
    """Make the current stream wait for every weight gradient launched so far (a no-op when there is none)."""
    for dev, st in list(_SIDE.items()):                      # (a second device's autograd thread may add its entry meanwhile)
        if st[0] is not None:
            cur = torch.cuda.current_stream(dev)
            cur.wait_stream(st[0])
            if st[1]:                                        # side work was launched since the last join: mark its end for the pacer
                if st[3] is None:
                    st[3] = torch.cuda.Event()
                st[3].record(cur)
        st[1] = False
        st[2].clear()


def _on_side(fn, w, *operands):
    dev = operands[0].device
    if (not WGRAD_OVERLAP or w is None or not w.is_leaf or w._backward_hooks or torch.cuda.is_current_stream_capturing()
            or torch.is_grad_enabled()          # backward(create_graph=True): AccumulateGrad CLONES the gradient on the main stream
            or not w.is_contiguous()):          # layout outside AccumulateGrad's stealing contract: it clones there too
        return fn()
    st = _SIDE.get(dev.index)
    if st is None:
        st = _SIDE[dev.index] = [torch.cuda.Stream(device=dev), False, set(), None]
    if w.grad is not None or w.data_ptr() in st[2]:
        # The weight already has a gradient (accumulation over several backward passes), or this pass has already produced one
        # for it (a layer used twice in one graph -- the reference calls its encoder once per image): autograd will ADD the
        # two on the main stream as soon as this node returns (AccumulateGrad, or the input buffer of the leaf's node), so
        # both operands of that addition must be complete there.
        join_side_streams()
        st[2].add(w.data_ptr())
        return fn()
    st[2].add(w.data_ptr())
    side, main = st[0], torch.cuda.current_stream(dev)
    if side == main:
        return fn()
    if not st[1]:
        pace_side_streams()               # first side launch of this pass: the previous pass's operands must have been released
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    for t in operands:
        t.record_stream(side)
    out.record_stream(main)
    if not st[1]:
        st[1] = True
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)
        except RuntimeError:              # not inside a backward pass (a direct call of backward()): join at once
            join_side_streams()
    return out


def _launch_pair(wfn, dfn):
    """Launch order of a layer's weight gradient (wfn, may go to the side stream) and data gradient (dfn, main stream).
    Weight gradient first: the side stream forks BEFORE the data gradient is queued, so the two start together.  The other
    order (ECM_WGRAD_FIRST=0: the side stream waits for the layer's own data gradient and the weight gradient starts with the
    GroupNorm backward that follows) measured 1 ms slower per backward pass (84.5 vs 83.5 ms at batch 4)."""
    if WGRAD_FIRST:
        gw = wfn() if wfn else None
        gx = dfn() if dfn else None
    else:
        gx = dfn() if dfn else None
        gw = wfn() if wfn else None
    return gx, gw


def _wino_wgrad(x, gy, Co, Ci, kd, w=None):
    """w: the weight tensor the gradient is for (decides whether the side stream may be used, see _on_side)."""
    return _on_side(lambda: _wino_wgrad_now(x, gy, Co, Ci, kd), w, x, gy)


def _wino_wgrad_now(x, gy, Co, Ci, kd):
    """Winograd-form weight gradient of a stride-1 3x3(x3) convolution: x [B,Ci,(D,)H,W], gy [B,Co,(D,)H,W]."""
    B = x.shape[0]
    D, H, W = (x.shape[2:] if x.dim() == 5 else (1,) + tuple(x.shape[2:]))
    gw = torch.empty((Co, Ci) + ((3, 3, 3) if kd == 3 else (3, 3)), device=x.device, dtype=x.dtype)
    _call_scratch(x.device, "ecm_conv_wino_wgrad_scratch_bytes", (B, Ci, Co, D, H, W, kd), "ecm_conv_wino_wgrad",
                  _p(x), _p(gy), _p(gw), _SCRATCH, B, Ci, Co, D, H, W, kd, _stream())
    return gw


def _wgrad(x, gy, Co, Ci, stride, w=None):
    """gw[Co,Ci,3,3,3] = sum gy[b,co,o] x[b,ci,o*stride+k-1]."""
    if stride == 1 and _wino_ok(x) and WINOGRAD_WGRAD:
        return _wino_wgrad(x, gy, Co, Ci, 3, w)
    return _on_side(lambda: _wgrad_direct(x, gy, Co, Ci, stride), w, x, gy)


def _wgrad_direct(x, gy, Co, Ci, stride):
    B, _, D, H, W = x.shape
    gw = torch.empty(Co, Ci, 3, 3, 3, device=x.device, dtype=x.dtype)
    _call_scratch(x.device, "ecm_conv3d_wgrad_scratch_bytes", (B, Ci, Co, D, H, W, stride), "ecm_conv3d_k3_wgrad",
                  _p(x), _p(gy), _p(gw), _SCRATCH, B, Ci, Co, D, H, W, stride, _stream())
    return gw


# The classifier's 32 -> 1 layer has its own kernels (conv3d_c1.hip).  With gn = (stats, gamma, beta) they read the RAW
# input of the GroupNorm + ReLU in front of the layer and normalise + rectify it while they stage it (ClassifierTail).
def _is_c1(w, stride):
    return w.shape[0] == 1 and stride == 1 and w.shape[1] <= 32 and w.shape[1] % 8 == 0


def _c1_fwd(x, w, gn=None):
    B, Ci, D, H, W = x.shape
    y = torch.empty(B, 1, D, H, W, device=x.device, dtype=x.dtype)
    if gn is None:
        _lib.call("ecm_conv3d_c1_fwd", _p(x), _p(w), _p(y), B, Ci, D, H, W, _stream())
    else:
        _lib.call("ecm_conv3d_c1_gn_fwd", _p(x), *map(_p, gn), _p(w), _p(y), B, Ci, D, H, W, _stream())
    return y


def _c1_dgrad(gy, w, x):
    """Gradient w.r.t. the layer's (normalised) input, of x's shape."""
    B, Ci, D, H, W = x.shape
    g = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _lib.call("ecm_conv3d_c1_dgrad", _p(gy), _p(w), _p(g), B, Ci, D, H, W, _stream())
    return g


def _c1_wgrad(x, gy, w, gn=None):
    B, Ci, D, H, W = x.shape
    g = _empty_like(w)
    name, xs = ("ecm_conv3d_c1_wgrad", (_p(x),)) if gn is None else ("ecm_conv3d_c1_gn_wgrad", (_p(x), *map(_p, gn)))
    _call_scratch(x.device, "ecm_conv3d_c1_wgrad_scratch_bytes", (B, Ci, D, H, W), name, *xs, _p(gy), _p(g), _SCRATCH,
                  B, Ci, D, H, W, _stream())
    return g


class Conv3dK3(torch.autograd.Function):
    """nn.Conv3d(k=3, pad=1, stride 1|2, bias=False) (cmfsm.py:52-57)."""

    @staticmethod
    def forward(ctx, x, w, stride, fork=False, grad_mode=True):
        _chk(x, w)
        _need(x.dim() == 5 and w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and w.shape[1] == x.shape[1] and stride in (1, 2)
              and x.numel() > 0 and w.shape[0] > 0,
              lambda: f"conv3d_k3: x {tuple(x.shape)}, w {tuple(w.shape)}, stride {stride}: want [B,Ci,D,H,W], [Co,Ci,3,3,3], stride 1|2")
        ctx.side_ok = w.is_contiguous()        # else the saved weight is a COPY and AccumulateGrad will re-lay the gradient out (see _on_side)
        x, w = _c(x), _c(w)
        ctx.set_materialize_grads(False)
        ctx.c1 = _is_c1(w, stride)
        if ctx.c1:
            y = _c1_fwd(x, w)
        elif stride == 1 and _wino_ok(x):
            y = _wino_run(x, _wino_pack_fwd(ctx, x, w, 3, grad_mode), w.shape[0], 3)
        elif stride == 2 and _split_use("conv_fwd", x, w.shape[1], w.shape[0]):
            y = _split_conv_fwd(x, _pack_split(w, False), w.shape[0])
        else:
            y = _conv_fwd(x, _pack_conv(w), w.shape[0], stride)
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        ctx.split_dgrad = stride == 2 and not ctx.c1 and _split_use("conv_dgrad", x, w.shape[0], w.shape[1])
        return _fork_out(y, x, fork)

    @staticmethod
    def backward(ctx, gy, gskip=None):
        x, w = ctx.saved_tensors
        if gy is None:                         # only the forked input was used downstream
            return gskip, None, None, None, None
        gy = _c(gy)
        Co, Ci = w.shape[0], w.shape[1]

        def wfn():
            if ctx.c1:
                return _c1_wgrad(x, gy, w)
            return _wgrad(x, gy, Co, Ci, ctx.stride, w if ctx.side_ok else None)

        def dfn():
            if ctx.c1:
                g = _c1_dgrad(gy, w, x)
            elif ctx.stride == 1 and _wino_ok(x):
                return _wino_run(gy, _wino_pack_b(ctx, w, 3), Ci, 3, addend=gskip)
            elif ctx.stride == 1:
                g = _conv_fwd(gy, _pack_conv(w, True), Ci, 1)
            elif ctx.split_dgrad:
                g = _split_deconv_fwd(gy, _pack_split(w, True), Ci, x.shape[2:])
            else:
                g = _deconv_fwd(gy, _pack_deconv(w), Ci, x.shape[2:])
            return _fork_grad(g, gskip)
        gx, gw = _launch_pair(wfn if ctx.needs_input_grad[1] else None, dfn if ctx.needs_input_grad[0] else None)
        return gx, gw, None, None, None


# Packed-weight cache.  Packing a weight is one small launch per layer and call; a training step changes every weight, so
# there is nothing to cache there, and by default every call packs afresh -- which also follows in-place updates that the
# version counter does not see (`p.data.copy_()`, `dist.broadcast(p.data)`, `m.weight.data.normal_()`), and puts the pack
# kernels INSIDE a captured HIP graph so that replays follow weight updates.  An evaluation loop over fixed weights may
# opt in with `with ops.frozen_weights(): ...`: inside it a packed layout rides on the weight tensor OBJECT, tagged with the
# context's epoch, the tensor's version counter and its storage address, and is reused until one of them moves; leaving the
# outermost context (or `invalidate_packed()`) drops every cached layout.  Keying a global table by data_ptr would be wrong:
# the caching allocator hands the same address to the next tensor of that size.
_FROZEN_DEPTH = 0
_PACK_EPOCH = 0


@_contextlib.contextmanager
def frozen_weights():
    """Promise that no weight is written inside the block by means the version counter misses (`.data` writes): packed
    weight layouts are then built once and reused (~60 fewer launches per eval forward of cmfsm)."""
    global _FROZEN_DEPTH, _PACK_EPOCH
    _FROZEN_DEPTH += 1
    try:
        yield
    finally:
        _FROZEN_DEPTH -= 1
        if _FROZEN_DEPTH == 0:
            _PACK_EPOCH += 1


def invalidate_packed():
    """Drop every cached packed layout (call after writing weights through `.data` inside a frozen_weights() block)."""
    global _PACK_EPOCH
    _PACK_EPOCH += 1


def _cached_pack(w, kind, build):
    if _FROZEN_DEPTH == 0 or torch.cuda.is_current_stream_capturing():
        return build()
    cache = getattr(w, "_ecm_packed", None)
    if cache is None:
        cache = {}
        try:
            w._ecm_packed = cache
        except AttributeError:
            return build()
    tag = (_PACK_EPOCH, w._version, w.data_ptr(), w.device)
    hit = cache.get(kind)
    if hit is not None and hit[0] == tag:
        return hit[1]
    packed = build()
    cache[kind] = (tag, packed)
    return packed


# (kh, kw, stride, dil) -> output-channel tilings (tiles of 32 per workgroup) the kernels are instantiated for; mirrors the
# COTS masks of csrc/conv2d_case_*.hip and the tiling rule c2_plan() of csrc/conv2d_kernel.h
_C2_CASES = {(3, 3, 1, 1): {1, 2, 3, 4}, (3, 3, 1, 2): {2, 4}, (3, 3, 1, 4): {4}, (3, 3, 2, 1): {1, 2, 3, 4},
             (3, 5, 1, 1): {1, 3}, (1, 1, 1, 1): {1, 2, 4}, (1, 1, 2, 1): {1, 2, 4}}


def _cot(Co, kh, kw):
    if Co <= 32:
        return 1
    if Co <= 64:
        return 2
    return 3 if (kh * kw != 1 and Co % 96 == 0 and Co % 128 != 0) else 4


def conv2d_supported(Ci, Co, kh, kw, stride, dil):
    """Is this layer -- forward AND data gradient -- inside the native 2-D family (csrc/conv2d.hip)?"""
    cots = _C2_CASES.get((kh, kw, stride, dil))
    if cots is None or _cot(Co, kh, kw) not in cots:
        return False
    if stride == 1:
        return _cot(Ci, kh, kw) in cots                      # data gradient: same case with Cout' = Ci
    if kh == 3:                                              # stride-2 3x3: transposed-conv kernel, <= 64 output channels
        return Ci <= 64 and Co % 4 == 0
    return _cot(Ci, 1, 1) in _C2_CASES[(1, 1, 1, 1)]         # stride-2 1x1: a stride-1 1x1 on the coarse grid + zero insertion


def _pack2d(w, flip_transpose):
    w = _c(w)
    Co, Ci, kh, kw = w.shape
    kin, kout = (Co, Ci) if flip_transpose else (Ci, Co)

    def build():
        packed = torch.empty(_lib.query("ecm_conv2d_packed_floats_ex", kin, kout, kh, kw), device=w.device, dtype=w.dtype)
        _lib.call("ecm_conv2d_pack_weight_ex", _p(w), _p(packed), Co, Ci, kh, kw, int(flip_transpose), _stream())
        return packed
    return _cached_pack(w, "c2T" if flip_transpose else "c2", build)


def _conv2d_run(x, packed, Co, kh, kw, stride, dil, pad_top, pad_left, Ho, Wo):
    B, Ci, H, W = x.shape
    y = torch.empty(B, Co, Ho, Wo, device=x.device, dtype=x.dtype)
    _lib.call("ecm_conv2d_fwd_ex", _p(x), _p(packed), _p(y), B, Ci, Co, H, W, kh, kw, stride, dil, pad_top, pad_left, Ho, Wo,
              _stream())
    return y


class Conv2dG(torch.autograd.Function):
    """nn.Conv2d(bias=False) of the encoder (convbn, cmfsm.py:36-46; 1x1 projections 152-170, 231-236) and the class
    convolutions of the collapsed cost volume, on the MFMA implicit-GEMM kernels: forward, data gradient (stride 1: the
    same kernel on flipped / transposed weights; stride 2: the transposed-conv kernel) and weight gradient."""

    @staticmethod
    def forward(ctx, x, w, stride, dil, pad_top, pad_left, Ho, Wo, fork=False, grad_mode=True):
        _chk(x, w)
        _need(x.dim() == 4 and w.dim() == 4 and w.shape[1] == x.shape[1] and x.numel() > 0 and w.shape[0] > 0
              and stride >= 1 and dil >= 1 and pad_top >= 0 and pad_left >= 0 and Ho >= 1 and Wo >= 1,
              lambda: f"conv2d: x {tuple(x.shape)}, w {tuple(w.shape)}, stride {stride}, dilation {dil}, pad ({pad_top}, {pad_left}), "
                      f"out ({Ho}, {Wo}): want [B,Ci,H,W] and [Co,Ci,kh,kw]")
        x = _c(x)
        ctx.set_materialize_grads(False)
        Co, Ci, kh, kw = w.shape
        same = (kh, kw, stride, dil, pad_top, pad_left) == (3, 3, 1, 1, 1, 1) and (Ho, Wo) == tuple(x.shape[-2:])
        # Winograd where it is ahead of the direct kernel (tools/wino_time.py): from 32 channels up (32->32 at 576x960:
        # 0.56 vs 0.73 ms); below that (the 3-channel stem) the 16 frequency planes are mostly padding
        ctx.wino_f, ctx.wino_b = _wino_ok(x) and same and Ci >= WINO2D_MIN_CI, _wino_ok(x) and same and Co >= WINO2D_MIN_CI
        ctx.wino_same = same
        if ctx.wino_f:
            y = _wino_run(x, _wino_pack_fwd(ctx, x, _c(w), 1, grad_mode), Co, 1)
        else:
            y = _conv2d_run(x, _pack2d(w, False), Co, kh, kw, stride, dil, pad_top, pad_left, Ho, Wo)
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, dil, pad_top, pad_left, Ho, Wo)
        return _fork_out(y, x, fork)

    @staticmethod
    def backward(ctx, gy, gskip=None):
        x, w = ctx.saved_tensors
        if gy is None:
            return (gskip,) + (None,) * 9
        stride, dil, pad_top, pad_left, Ho, Wo = ctx.cfg
        Co, Ci, kh, kw = w.shape
        B, _, H, W = x.shape
        gy = _c(gy)
        def wfn():
            if ctx.wino_same and _wino_ok(x) and WINOGRAD_WGRAD:
                return _wino_wgrad(x, gy, Co, Ci, 1, w)

            def direct():
                g = _empty_like(w)
                _call_scratch(x.device, "ecm_conv2d_wgrad_ex_scratch_bytes", (B, Ci, Co, Ho, Wo, kh, kw, stride),
                              "ecm_conv2d_wgrad_ex", _p(x), _p(gy), _p(g), _SCRATCH, B, Ci, Co, H, W, kh, kw, stride, dil,
                              pad_top, pad_left, Ho, Wo, _stream())
                return g
            return _on_side(direct, w, x, gy)

        def dfn():
            if ctx.wino_b:
                return _wino_run(gy, _wino_pack_b(ctx, _c(w), 1), Ci, 1, addend=gskip)
            if stride == 1:
                # gx[i] = sum_k w[k] gy[i + pad - k*dil]: the conv of gy with the flipped kernel, padding (K-1)*dil - pad
                g = _conv2d_run(gy, _pack2d(w, True), Ci, kh, kw, 1, dil, (kh - 1) * dil - pad_top, (kw - 1) * dil - pad_left,
                                H, W)
            elif kh == 3:
                if pad_top != 1 or pad_left != 1:
                    raise RuntimeError("stride-2 3x3 data gradient: padding 1 only")
                wc = _c(w)

                def build():
                    packed = torch.empty(9 * Co * ((Ci + 31) // 32) * 32, device=w.device, dtype=w.dtype)
                    _lib.call("ecm_deconv2d_pack_weight", _p(wc), _p(packed), Co, Ci, _stream())
                    return packed
                g = torch.empty(B, Ci, H, W, device=x.device, dtype=x.dtype)
                _lib.call("ecm_deconv2d_k3s2_fwd", _p(gy), _p(_cached_pack(wc, "d2", build)), _p(g), B, Co, Ci, Ho, Wo, H, W,
                          _stream())
            else:
                # 1x1, stride 2 (the downsample projections): W^T gy lands on the even positions, zeros elsewhere
                small = _conv2d_run(gy, _pack2d(w, True), Ci, 1, 1, 1, 1, 0, 0, Ho, Wo)
                g = torch.empty(B, Ci, H, W, device=x.device, dtype=x.dtype)
                _lib.call("ecm_zero_insert2d", _p(small), _p(g), C.c_longlong(B * Ci), H, W, Ho, Wo, _stream())
            return _fork_grad(g, gskip)
        gx, gw = _launch_pair(wfn if ctx.needs_input_grad[1] else None, dfn if ctx.needs_input_grad[0] else None)
        return gx, gw, None, None, None, None, None, None, None, None


def conv2d(x, w, stride=1, dil=1, pad_top=None, pad_left=None, Ho=None, Wo=None, fork=False):
    """General native 2-D convolution; default padding "same-style" dil*(k-1)/2 and the matching output size.
    fork=True: returns (y, x') with x' a view of x to be used as the skip operand (see _fork_out)."""
    kh, kw = w.shape[-2:]
    H, W = x.shape[-2:]
    pt = dil * (kh - 1) // 2 if pad_top is None else int(pad_top)
    pl = dil * (kw - 1) // 2 if pad_left is None else int(pad_left)
    if Ho is None:
        Ho = (H + 2 * pt - dil * (kh - 1) - 1) // stride + 1
    if Wo is None:
        Wo = (W + 2 * pl - dil * (kw - 1) - 1) // stride + 1
    return Conv2dG.apply(x, w, int(stride), int(dil), pt, pl, int(Ho), int(Wo), bool(fork), torch.is_grad_enabled())


def conv2d_k3(x, w):
    """3x3 / stride 1 / pad 1 (kept as the name the 32/64-channel encoder layers were introduced under)."""
    return conv2d(x, w, 1, 1)


# ---- dilated 3x3 layers as d*d independent phase planes ---------------------------------------------------------------------
# A dilation-d 3x3 convolution (padding d) touches only pixels of equal (y mod d, x mod d): it is d*d independent ordinary
# 3x3 / pad 1 convolutions of the phase sub-images x[..., p::d, q::d].  A layer whose convolutions all have dilation d
# (cmfsm's layer4, cmfsm.py:150: 128 -> 128, dilation 2) therefore runs on the Winograd kernels with its activations kept as
# [B,C,d*d,H/d,W/d] (GroupNorm and the residual adds see the same elements in another order), at the price of one
# re-arrangement on the way in and one on the way out.
def phase_split(x, d):
    B, Cc, H, W = x.shape
    return x.view(B, Cc, H // d, d, W // d, d).permute(0, 1, 3, 5, 2, 4).reshape(B, Cc, d * d, H // d, W // d)


def phase_merge(x, d):
    B, Cc, _, h, w = x.shape
    return x.view(B, Cc, d, d, h, w).permute(0, 1, 4, 2, 5, 3).reshape(B, Cc, h * d, w * d)


class Conv2dPlanes(torch.autograd.Function):
    """3x3 / stride 1 / pad 1 Conv2d applied to every plane of x [B,Ci,P,h,w] (P = the phase planes of a dilated layer) on
    the Winograd kernels: forward, data gradient and weight gradient."""

    @staticmethod
    def forward(ctx, x, w, fork=False, grad_mode=True):
        _chk(x, w)
        _need(x.dim() == 5 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and w.shape[1] == x.shape[1] and x.numel() > 0
              and w.shape[0] > 0 and _wino_ok(x),
              lambda: f"conv2d_planes: x {tuple(x.shape)}, w {tuple(w.shape)}: want [B,Ci,P,h,w] and [Co,Ci,3,3] (Winograd path)")
        ctx.side_ok = w.is_contiguous()
        x, w = _c(x), _c(w)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, w)
        return _fork_out(_wino_run(x, _wino_pack_fwd(ctx, x, w, 1, grad_mode), w.shape[0], 1), x, fork)

    @staticmethod
    def backward(ctx, gy, gskip=None):
        x, w = ctx.saved_tensors
        if gy is None:
            return gskip, None, None, None
        gy = _c(gy)
        gx, gw = _launch_pair((lambda: _wino_wgrad(x, gy, w.shape[0], w.shape[1], 1, w if ctx.side_ok else None)) if ctx.needs_input_grad[1] else None,
                              (lambda: _wino_run(gy, _wino_pack_b(ctx, w, 1), w.shape[1], 1, addend=gskip)) if ctx.needs_input_grad[0] else None)
        return gx, gw, None, None


def conv2d_planes(x, w, fork=False):
    return Conv2dPlanes.apply(x, w, bool(fork), torch.is_grad_enabled())


def conv3d_k3(x, w, stride=1, fork=False):
    """fork=True: returns (y, x') with x' a view of x to be used as the skip operand (see _fork_out).
    A bf16 x runs the bf16 inference kernel (see aggregation_dtype)."""
    if x.dtype == torch.bfloat16:
        return _conv3d_bf16(x, w, int(stride), bool(fork))
    _AGG.guard("conv3d_k3")
    return Conv3dK3.apply(x, w, int(stride), bool(fork), torch.is_grad_enabled())


class Deconv3dK3S2(torch.autograd.Function):
    """nn.ConvTranspose3d(k=3, stride=2, pad=1, output_padding=1, bias=False) (cmfsm.py:262-268)."""

    @staticmethod
    def forward(ctx, x, w):
        _chk(x, w)
        _need(x.dim() == 5 and w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and w.shape[0] == x.shape[1] and x.numel() > 0
              and w.shape[1] > 0,
              lambda: f"deconv3d_k3s2: x {tuple(x.shape)}, w {tuple(w.shape)}: want [B,Ci,D,H,W] and ConvTranspose3d's [Ci,Co,3,3,3]")
        ctx.side_ok = w.is_contiguous()
        x, w = _c(x), _c(w)
        B, Ci, D, H, W = x.shape
        if _split_use("deconv_fwd", x, w.shape[0], w.shape[1]):
            y = _split_deconv_fwd(x, _pack_split(w, True), w.shape[1], (2 * D, 2 * H, 2 * W))
        else:
            y = _deconv_fwd(x, _pack_deconv(w), w.shape[1], (2 * D, 2 * H, 2 * W))
        ctx.save_for_backward(x, w)
        ctx.split_dgrad = _split_use("deconv_dgrad", x, w.shape[1], w.shape[0])
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _c(gy)
        Ci, Co = w.shape[0], w.shape[1]
        # gw[ci,co,k] = sum x[ci,i] gy[co,2i+k-1]: the conv-wgrad with x:=gy (big), gy:=x, "Co":=Ci, "Ci":=Co
        # gx[ci,i] = sum_{co,k} gy[co,2i+k-1] w[ci,co,k]: a stride-2 conv with w read as Conv3d [Cout=Ci,Cin=Co]
        def dfn():
            if ctx.split_dgrad:
                return _split_conv_fwd(gy, _pack_split(w, False), Ci)
            return _conv_fwd(gy, _pack_conv(w), Ci, 2)
        gx, gw = _launch_pair((lambda: _wgrad(gy, x, Ci, Co, 2, w if ctx.side_ok else None)) if ctx.needs_input_grad[1] else None,
                              dfn if ctx.needs_input_grad[0] else None)
        return gx, gw


def deconv3d_k3s2(x, w):
    if x.dtype == torch.bfloat16:
        return _deconv3d_bf16(x, w)
    _AGG.guard("deconv3d_k3s2")
    return Deconv3dK3S2.apply(x, w)


# ---- cmf decoder (super_resolution_refinement, cmf.py:227-264) --------------------------------------------------------------
def channel_sum(x):
    """[B,C,...] -> [C]: sum over everything but the channel axis in a fixed order (the bias gradient of a layer; no atomics)."""
    _chk(x)
    x = _c(x)
    B, Cc = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * Cc, 1)
    out = torch.empty(Cc, device=x.device, dtype=x.dtype)
    _call_scratch(x.device, "ecm_channel_sum_scratch_bytes", (B, Cc, C.c_longlong(HW)), "ecm_channel_sum",
                  _p(x), _p(out), _SCRATCH, B, Cc, C.c_longlong(HW), _stream())
    return out


class Deconv2dK3S2Bias(torch.autograd.Function):
    """nn.ConvTranspose2d(Ci, Co, 3, stride 2, pad 1, output_padding 1, bias=True) (cmf.py:236-239): forward with the bias in
    the kernel's epilogue; data gradient = the stride-2 3x3 Conv2d of gy with the weight read as a Conv2d [Ci,Co,3,3] (COT-3
    case for Ci = 96); weight gradient = the 2-D conv-wgrad with the roles of x and gy exchanged; bias gradient =
    channel_sum(gy)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _chk(x, w, b)
        _need(x.dim() == 4 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and w.shape[0] == x.shape[1] and x.numel() > 0
              and b.dim() == 1 and b.shape[0] == w.shape[1] and w.shape[1] <= 64 and x.shape[1] % 4 == 0,
              lambda: f"deconv2d_k3s2_bias: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}: want [B,Ci,H,W], "
                      "ConvTranspose2d's [Ci,Co<=64,3,3] with Ci % 4 == 0 and [Co]")
        x, w, b = _c(x), _c(w), _c(b)
        B, Ci, H, W = x.shape
        Co = w.shape[1]

        def build():
            packed = torch.empty(9 * Ci * ((Co + 31) // 32) * 32, device=w.device, dtype=w.dtype)
            _lib.call("ecm_deconv2d_pack_weight", _p(w), _p(packed), Ci, Co, _stream())
            return packed
        y = torch.empty(B, Co, 2 * H, 2 * W, device=x.device, dtype=x.dtype)
        _lib.call("ecm_deconv2d_k3s2_bias_fwd", _p(x), _p(_cached_pack(w, "d2b", build)), _p(b), _p(y), B, Ci, Co, H, W, 2 * H,
                  2 * W, _stream())
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _c(gy)
        B, Ci, H, W = x.shape
        Co, Ho, Wo = w.shape[1], 2 * H, 2 * W
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # gx[ci,i] = sum_{co,k} gy[co,2i+k-1] w[ci,co,k]: a Conv2d(Co -> Ci, stride 2, pad 1) with weight [Ci,Co,3,3]
            gx = _conv2d_run(gy, _pack2d(w, False), Ci, 3, 3, 2, 1, 1, 1, H, W)
        if ctx.needs_input_grad[1]:
            # gw[ci,co,k] = sum x[ci,i] gy[co,2i+k-1]: the conv-wgrad with x := gy, gy := x, "Co" := Ci, "Ci" := Co
            gw = _empty_like(w)
            _call_scratch(x.device, "ecm_conv2d_wgrad_ex_scratch_bytes", (B, Co, Ci, H, W, 3, 3, 2), "ecm_conv2d_wgrad_ex",
                          _p(gy), _p(x), _p(gw), _SCRATCH, B, Co, Ci, Ho, Wo, 3, 3, 2, 1, 1, 1, H, W, _stream())
        if ctx.needs_input_grad[2]:
            gb = channel_sum(gy)
        return gx, gw, gb


def deconv2d_k3s2_bias(x, w, b):
    return Deconv2dK3S2Bias.apply(x, w, b)


class Conv2dC1Relu(torch.autograd.Function):
    """relu(nn.Conv2d(Ci, 1, 3, 1, 1, bias=True)(x)) (cmf.py:259-264, conv_out + crap) on csrc/conv2d_c1.hip: forward with
    bias and ReLU fused, data gradient with the ReLU mask applied, weight and bias gradient in one deterministic pass."""

    @staticmethod
    def forward(ctx, x, w, b):
        _chk(x, w, b)
        _need(x.dim() == 4 and tuple(w.shape) == (1, x.shape[1], 3, 3) and b.numel() == 1 and x.numel() > 0,
              lambda: f"conv2d_c1_relu: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}: want [B,Ci,H,W], "
                      "[1,Ci,3,3] and [1]")
        x, w, b = _c(x), _c(w), _c(b)
        B, Ci, H, W = x.shape
        y = torch.empty(B, 1, H, W, device=x.device, dtype=x.dtype)
        _lib.call("ecm_conv2d_c1_fwd", _p(x), _p(w), _p(b), _p(y), B, Ci, H, W, _stream())
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gy = _c(gy)
        B, Ci, H, W = x.shape
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.call("ecm_conv2d_c1_dgrad", _p(gy), _p(y), _p(w), _p(gx), B, Ci, H, W, _stream())
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw = _empty_like(w)
            gb = torch.empty(1, device=x.device, dtype=x.dtype)
            _call_scratch(x.device, "ecm_conv2d_c1_wgrad_scratch_bytes", (B, Ci, H, W), "ecm_conv2d_c1_wgrad",
                          _p(x), _p(gy), _p(y), _p(gw), _p(gb), _SCRATCH, B, Ci, H, W, _stream())
        return gx, gw, gb


def conv2d_c1_relu(x, w, b):
    return Conv2dC1Relu.apply(x, w, b)


# Exchange memory of the one-pass GroupNorm kernels (cluster slots, ticket counter, per-span counters): kept per (device,
# stream), preset once; the kernels hand it back in the preset state, so no memset precedes a launch (include/ecm_hip.h:
# ecm_gn3d_fwd_p).  Dropped -- hence preset afresh -- whenever a call fails or an asynchronous time-out is reported.
_GN_CLUSTER = {}


def _gn_cluster(B, device):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    nb = _lib.query("ecm_gn3d_cluster_bytes", B)
    buf = _GN_CLUSTER.get(key)
    if buf is None or buf.numel() < nb:
        buf = torch.empty(max(int(nb), 1 << 20), dtype=torch.uint8, device=device)
        _lib.call("ecm_gn3d_cluster_preset", _p(buf), C.c_longlong(buf.numel()), _stream())
        _GN_CLUSTER[key] = buf
    return buf


def _gn_call(name, *args):
    try:
        _lib.call(name, *args)
    except RuntimeError:
        _GN_CLUSTER.clear()
        raise


def _gn_capturing():
    """During HIP-graph capture the kept exchange buffer must not be used: `torch.cuda.graph` captures on ONE
    stream for every graph, so the (device, stream) cache would hand a buffer that was allocated in -- and preset by -- the
    FIRST graph to every later capture, whose kernels would then depend on another graph's replay having run (and two graphs
    replayed concurrently would share the buffer).  A captured GroupNorm therefore takes the stateless entry points
    (ecm_gn3d_fwd / _bwd), and the library itself gives a capturing stream the two-stage kernels -- no inter-workgroup
    waits, no exchange memory -- because two graphs replayed concurrently could otherwise starve each other's clusters
    (csrc/gn3d.hip: GnControl)."""
    return torch.cuda.is_current_stream_capturing()


def _gn_launch(stateless, kept, x, front, back):
    """One fp32 GroupNorm launch: outside capture the entry point `kept` on the kept exchange memory (_gn_cluster), during
    capture the `stateless` one (_gn_capturing).  front: the pointer arguments, which the scratch pair [and the exchange
    pair] follow;  back: the arguments after (B, C, S)."""
    B, Cc = x.shape[:2]
    S = x.numel() // (B * Cc)
    name, cl = stateless, ()
    if not _gn_capturing():
        buf = _gn_cluster(B, x.device)
        name, cl = kept, (_p(buf), C.c_longlong(buf.numel()))
    _call_scratch(x.device, "ecm_gn3d_scratch_bytes", (B, Cc, C.c_longlong(S)), name, *front, _SCRATCH, *cl,
                  B, Cc, C.c_longlong(S), *back, _stream(), call=_gn_call)


def _gn_fwd(x, gamma, beta, skip, relu):
    """-> (y, stats [B,32,2]) of y = relu?(GroupNorm32(x)*gamma+beta (+ skip))."""
    stats = torch.empty(x.shape[0], GN_GROUPS, 2, device=x.device, dtype=x.dtype)
    y = _empty_like(x)
    _gn_launch("ecm_gn3d_fwd", "ecm_gn3d_fwd_p", x, (_p(x), _p(gamma), _p(beta), _p(skip), _p(y), _p(stats)),
               (int(relu), float(GN_EPS)))
    return y, stats


def _gn_bwd(x, stats, gamma, beta, y, gy, gskip_out, relu):
    """Backward of _gn_fwd -> (gx, ggamma, gbeta).  y: the forward's output where the ReLU mask needs it (a skip was added),
    else None (the mask is recomputed from x);  gskip_out: the tensor that receives the masked skip gradient, or None."""
    gx = _empty_like(x)
    ggamma, gbeta = _empty_like(gamma), _empty_like(gamma)
    _gn_launch("ecm_gn3d_bwd", "ecm_gn3d_bwd_p", x, (_p(x), _p(stats), _p(gamma), _p(beta), _p(y), _p(gy), _p(gx),
                                                    _p(gskip_out), _p(ggamma), _p(gbeta)), (int(relu),))
    return gx, ggamma, gbeta


class GroupNormAct(torch.autograd.Function):
    """y = relu?( GroupNorm32(x)*gamma+beta (+ skip) )  (cmfsm.py:58 + ReLU/residual at 287-299, 606-613, 685-693)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, skip, relu, head=0):
        """head > 0 (a fork, cf. _fork_out): also returns x[:head] for a second consumer of the first `head` samples of the
        INPUT (the encoder's full-resolution map: the ECM weights read the left images' half, cmfsm.py:657-664); backward adds
        that consumer's gradient into the first `head` samples of gx -- a tensor this node has just produced and nobody else
        has seen, so the in-place add cannot touch memory another holder relies on."""
        _chk(x, gamma, beta, skip)
        _need(x.dim() >= 3 and x.numel() > 0 and x.shape[1] % GN_GROUPS == 0 and gamma.numel() == x.shape[1] == beta.numel()
              and (skip is None or skip.shape == x.shape) and 0 <= head <= x.shape[0],
              lambda: f"group_norm_act: x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, beta {tuple(beta.shape)}, skip "
                      f"{None if skip is None else tuple(skip.shape)}, head {head}: {GN_GROUPS} groups over C channels, skip of x's shape")
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        skip = _c(skip) if skip is not None else None
        y, stats = _gn_fwd(x, gamma, beta, skip, relu)
        # ReLU mask in backward: recomputed from x unless a skip was added (then the output y is needed)
        ctx.save_for_backward(x, stats, gamma, beta, y if (relu and skip is not None) else None)
        ctx.relu, ctx.has_skip, ctx.head = relu, skip is not None, int(head)
        if head:
            ctx.set_materialize_grads(False)
            return y, x[:head]
        return y

    @staticmethod
    def backward(ctx, gy, g_head=None):
        x, stats, gamma, beta, y = ctx.saved_tensors
        if gy is None:
            raise RuntimeError("GroupNormAct: the normalised output produced no gradient")     # not a configuration of these models
        gy = _c(gy)
        gskip = None
        if ctx.has_skip:                    # no mask: the skip gradient is gy itself (the same tensor: nobody writes a gradient in place)
            gskip = _empty_like(x) if ctx.relu else gy
        gx, ggamma, gbeta = _gn_bwd(x, stats, gamma, beta, y, gy, gskip if (ctx.has_skip and ctx.relu) else None, ctx.relu)
        if g_head is not None:
            gx[:ctx.head].add_(g_head)          # gx is this node's own fresh output (see forward)
        return gx, ggamma, gbeta, gskip, None, None


class ClassifierTail(torch.autograd.Function):
    """GroupNorm(32) + ReLU + Conv3d(32 -> 1, k3, pad 1) of a classifier (cmfsm.py:621-634: classifN[0][1], classifN[1],
    classifN[2]) with the normalised tensor never materialised: x [B,32,D,H,W] is the RAW output of classifN[0][0]; one read
    pass gives the group statistics (ecm_gn3d_stats) and the 32 -> 1 kernels normalise + rectify while they stage x
    (ecm_conv3d_c1_gn_fwd / _gn_wgrad).  Saves the GroupNorm kernel's write and the convolution's read of the 849 MB tensor
    (batch 4) per head, and the tensor itself.  Backward: gh = dgrad(gy) (w.r.t. the normalised tensor), the GroupNorm backward
    with the ReLU mask recomputed from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w):
        _chk(x, gamma, beta, w)
        _need(x.dim() == 5 and x.numel() > 0 and gamma.numel() == 32 == beta.numel(),
              lambda: f"classifier_tail: x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, beta {tuple(beta.shape)}")
        x, gamma, beta, w = _c(x), _c(gamma), _c(beta), _c(w)
        if x.shape[1] != 32 or tuple(w.shape) != (1, 32, 3, 3, 3):
            raise RuntimeError(f"classifier_tail: x {tuple(x.shape)}, w {tuple(w.shape)}: the fused tail exists for 32 -> 1 only")
        stats = _gn_stats(x)
        y = _c1_fwd(x, w, (stats, gamma, beta))
        ctx.save_for_backward(x, stats, gamma, beta, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, gamma, beta, w = ctx.saved_tensors
        gy = _c(gy)
        gn = (stats, gamma, beta)
        gh, gw = _launch_pair((lambda: _on_side(lambda: _c1_wgrad(x, gy, w, gn), w, x, gy, *gn)) if ctx.needs_input_grad[3] else None,
                              lambda: _c1_dgrad(gy, w, x))
        gx, ggamma, gbeta = _gn_bwd(x, stats, gamma, beta, None, gh, None, True)
        return gx, ggamma, gbeta, gw


def classifier_tail(x, gamma, beta, w):
    """relu(GroupNorm32(x)) -> Conv3d(32 -> 1): see ClassifierTail.  A bf16 x gives the same fp32 logits from the bf16 volume."""
    if x.dtype == torch.bfloat16:
        return _classifier_tail_bf16(x, gamma, beta, w)
    _AGG.guard("classifier_tail")
    return ClassifierTail.apply(x, gamma, beta, w)


FLYING3D_MEAN, FLYING3D_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # cmf/loader/Flying3d.py:26-27
_NORM3_OWN = {id(v): _host(C.c_float, v) for v in (FLYING3D_MEAN, FLYING3D_STD)}    # the defaults' host arrays: built and checked once


def frame_prep(frames, crop_y0, crop_x0, th, tw, split=None, tail=0, mean=FLYING3D_MEAN, std=FLYING3D_STD, want_image=False):
    """Batched GPU form of Flying3d.__getitem__ + transform (cmf/loader/Flying3d.py:49-99): frames [B,H,W,7] float32
    (resident) -> left, right [B,3,th,tw] normalised, disparity [B,th,tw] (and the raw left image in CHW).
    Train: th, tw = 256, 512 and crop_y0/crop_x0 = the window origins the loader draws at random.  Eval on 540x960 frames:
    th, tw = 576, 960, crops 0, split=540, tail=36 (the last 36 rows are appended again).
    `frames` may also be a packed shard: a tuple (rgb6 uint8 [B,H,W,6], disparity fp16|fp32 [B,H,W])."""
    return _frame_prep(frames, crop_y0, crop_x0, th, tw, split, tail, mean, std, want_image, 0)


def frame_prep_kitti_eval(frames, th=384, tw=1248, mean=FLYING3D_MEAN, std=FLYING3D_STD, want_image=False):
    """KITTI.__getitem__'s eval branch (cmf/loader/KITTI.py:98-108): top / left repeat padding to th x tw with the
    disparity zeroed in (and, through the loader's numpy views, next to) the padding.  `frames`: float32 [B,H,W,7] or a
    packed shard tuple as in frame_prep."""
    return _frame_prep(frames, None, None, th, tw, None, 0, mean, std, want_image, 1)


# ---- the operands of the frame decodes, stated once: the library reads B origins and 3 floats whatever a list holds
def _packed_shard(who, frames):                               # -> rgb6, disparity (contiguous), B, H, W of a shard that is not empty and on one device
    rgb, dsp = frames
    _on_device(rgb, dsp)
    _need(rgb.dtype == torch.uint8 and dsp.dtype in (torch.float16, torch.float32) and rgb.dim() == 4 and rgb.shape[-1] == 6
          and tuple(rgb.shape[:3]) == tuple(dsp.shape) and rgb.numel() > 0 and rgb.device == dsp.device,
          lambda: f"{who}: packed shard must be (uint8 [B,H,W,6], fp16|fp32 [B,H,W]) on one device, got {rgb.dtype} {tuple(rgb.shape)} "
                  f"on {rgb.device} / {dsp.dtype} {tuple(dsp.shape)} on {dsp.device}")
    return (rgb.contiguous(), dsp.contiguous(), *dsp.shape)


def _window_origins(who, crop_y0, crop_x0, B):
    ys, xs = [int(v) for v in (() if crop_y0 is None else crop_y0)], [int(v) for v in (() if crop_x0 is None else crop_x0)]
    if len(ys) != B or len(xs) != B:
        raise ValueError(f"{who}: crop_y0 {ys} / crop_x0 {xs}: one window origin per sample, {B} of each")
    return ys, xs


def _norm3(who, name, values, nonzero=False):                 # mean or std, any sequence of three finite numbers, as the host array an entry reads
    if id(values) in _NORM3_OWN:                               # the module's own constants, finite and non-zero: no check per batch
        return _NORM3_OWN[id(values)]
    vals = values.tolist() if hasattr(values, "tolist") else values
    if not isinstance(vals, (tuple, list)) or len(vals) != 3 or not all(_is_real(v) and not (nonzero and v == 0) for v in vals):
        raise ValueError(f"{who}: {name} {values!r}: three finite numbers" + (", none zero" if nonzero else ""))
    return _host(C.c_float, vals)


def _decode_outputs(B, rows, cols, dev, want_image, with_disp=True):
    left = torch.empty(B, 3, rows, cols, device=dev, dtype=torch.float32)
    disp = torch.empty(B, rows, cols, device=dev, dtype=torch.float32) if with_disp else None
    return left, torch.empty_like(left), disp, torch.empty_like(left) if want_image else None


def _decoded(left, right, disp, image):
    return (left, right, disp) if image is None else (left, right, disp, image)


def _frame_prep(frames, crop_y0, crop_x0, th, tw, split, tail, mean, std, want_image, mode):
    who, packed = "frame_prep", isinstance(frames, (tuple, list))
    if packed:
        rgb, dsp, B, H, W = _packed_shard(who, frames)
    else:
        _chk(frames)
        frames = _c(frames)
        B, H, W, ch = frames.shape
        if ch != 7:
            raise RuntimeError(f"frame_prep expects [B,H,W,7] frames (left RGB, right RGB, disparity), got {tuple(frames.shape)}")
    split = th if split is None else int(split)
    ys, xs = map(_host, (C.c_int, C.c_int), _window_origins(who, crop_y0, crop_x0, B)) if mode == 0 else (None, None)
    m3, s3 = _norm3(who, "mean", mean), _norm3(who, "std", std)
    left, right, disp, image = _decode_outputs(B, th, tw, rgb.device if packed else frames.device, want_image)
    outs = (_p(left), _p(right), _p(disp), _p(image), B, H, W)
    if packed:
        _lib.call("ecm_frame_prep_packed", _p(rgb), _p(dsp), int(dsp.dtype == torch.float16), *outs, ys, xs, int(th), int(tw), split, int(tail), m3, s3, mode, _stream())
    elif mode == 1:
        _lib.call("ecm_frame_prep_kitti_eval", _p(frames), *outs, int(th), int(tw), m3, s3, _stream())
    else:
        _lib.call("ecm_frame_prep", _p(frames), *outs, ys, xs, int(th), int(tw), split, int(tail), m3, s3, _stream())
    return _decoded(left, right, disp, image)


# ------------------------------------------------------------------------------------ the KITTI training transform
# DESIGN.md section 37; include/ecm_augment.h states every operation.  KITTI.transform's train branch (cmf/loader/KITTI.py:144-191)
# per view: ColorJitter(0.4, 0.4, 0.4, 0.4) on the PIL image, the PCA "lighting" shift, clamp to 0..1, normalise.  The jitter is
# Pillow's arithmetic on uint8, byte for byte (tests/golden/g13_jitter.npz); what torchvision 0.2 adds around it -- the ranges
# drawn, the shuffle, adjust_hue's uint8 wrap -- is restated from its source, not executed.  Forward only.
KITTI_JITTER = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.4, alphastd=0.1)                  # KITTI.py:20,164
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3                             # the codes of an order
_PCA_EIGVAL = (0.2175, 0.0188, 0.0045)                                                                    # KITTI.py:21
_PCA_EIGVEC = ((-0.5675, 0.7192, 0.4009), (-0.5808, -0.0045, -0.8140), (-0.5836, -0.6948, 0.4203))        # KITTI.py:22-26
_JITTER_MAX_PIXELS = 1 << 24


@dataclasses.dataclass
class JitterParams:
    """The drawn parameters of a batch, CPU tensors, view 0 = left and 1 = right: factors [B,2,3] fp32 (brightness, contrast,
    saturation), order [B,2,4] int32 (the codes of the operations present, in the order they run, then -1), hue_shift [B,2]
    int32 in 0..255, pca [B,2,3] fp32 (the shift added to the 0..1 image per channel)."""
    factors: torch.Tensor
    order: torch.Tensor
    hue_shift: torch.Tensor
    pca: torch.Tensor


def jitter_params(batch, rng, gen, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.4, alphastd=0.1):
    """Draw KITTI.transform's parameters for `batch` samples, the left view and then the right one of each, as torchvision 0.2's
    ColorJitter.get_params and KITTI.py's Lighting do: uniform(max(0, 1 - x), 1 + x) for brightness, contrast and saturation,
    uniform(-hue, hue) for the hue (stored as adjust_hue's uint8 wrap, trunc(h * 255) mod 256), a shuffle of the operations
    present (a strength of 0 omits its operation), and alpha ~ N(0, alphastd) three times for the PCA shift, formed by the
    loader's own torch statements.  rng is a random.Random, gen a CPU torch.Generator: the caller's, so the draws repeat with
    their seeds (the reference draws from global generators inside DataLoader workers; its stream is not matched)."""
    who = "jitter_params"
    batch = _integer(who, "batch", batch, 1, None)
    strengths = [_real(who, n, v, ">= 0") for n, v in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation))]
    hue, alphastd = _real(who, "hue", hue, ">= 0"), _real(who, "alphastd", alphastd, ">= 0")
    if hue > 0.5:
        raise ValueError(f"{who}: hue {hue}: at most 0.5, as torchvision's")
    if not isinstance(rng, random.Random) or not isinstance(gen, torch.Generator):
        raise ValueError(f"{who}: rng {type(rng).__name__}, gen {type(gen).__name__}: a random.Random and a torch.Generator")
    factors, order = torch.ones(batch, 2, 3, dtype=torch.float32), torch.full((batch, 2, 4), -1, dtype=torch.int32)
    shift, pca = torch.zeros(batch, 2, dtype=torch.int32), torch.zeros(batch, 2, 3, dtype=torch.float32)
    eigval, eigvec = torch.Tensor(_PCA_EIGVAL), torch.Tensor(_PCA_EIGVEC)
    for b in range(batch):
        for view in range(2):
            present = []
            for code, x in enumerate(strengths):
                if x > 0:
                    factors[b, view, code] = rng.uniform(max(0, 1 - x), 1 + x)
                    present.append(code)
            if hue > 0:
                shift[b, view] = int(rng.uniform(-hue, hue) * 255) % 256
                present.append(JITTER_HUE)
            rng.shuffle(present)
            order[b, view, :len(present)] = torch.tensor(present, dtype=torch.int32)
            if alphastd > 0:                                               # KITTI.py:29-36
                alpha = torch.empty(3).normal_(0, alphastd, generator=gen)
                pca[b, view] = eigvec.clone().mul(alpha.view(1, 3).expand(3, 3)).mul(eigval.view(1, 3).expand(3, 3)).sum(1).squeeze()
    return JitterParams(factors, order, shift, pca)


def jitter_tile():
    """The pixels of one tile of the contrast reduction (a query of the library: no GPU needed)."""
    return int(_lib.query("ecma_jitter_tile"))


def _jitter_views(who, views, factors, order, hue_shift, pca=None):
    """The per-view parameters as flat host lists, refused with ValueError where the library would refuse them."""
    def flat(name, v, shape, dtype):
        t = torch.as_tensor(v).detach().cpu()
        if tuple(t.shape) != shape or (t.is_floating_point() and not dtype.is_floating_point) or t.dtype == torch.bool or t.is_complex():
            raise ValueError(f"{who}: {name} {tuple(t.shape)} {t.dtype}: want {shape} of {'floats' if dtype.is_floating_point else 'integers'}")
        return t.to(torch.float64 if dtype.is_floating_point else torch.int64).reshape(views, -1)
    f = flat("factors", factors, (views, 3), torch.float32)
    o, h = flat("order", order, (views, 4), torch.int32), flat("hue_shift", hue_shift, (views,), torch.int32)
    if not bool(torch.isfinite(f).all()) or bool((f < 0).any()) or bool((f > _FLT_MAX).any()):
        raise ValueError(f"{who}: factors: finite fp32 values >= 0")
    for v, row in enumerate(o.tolist()):
        codes = [c for c in row if c != -1]
        if row[len(codes):] != [-1] * (4 - len(codes)) or any(c < 0 or c > 3 for c in codes) or len(set(codes)) != len(codes):
            raise ValueError(f"{who}: order {row} of view {v}: distinct codes 0..3, then -1")
    if bool((h < 0).any()) or bool((h > 255).any()):
        raise ValueError(f"{who}: hue_shift: 0..255")
    out = [_host(C.c_float, f.reshape(-1).tolist()), _host(C.c_int, o.reshape(-1).tolist()), _host(C.c_int, h.reshape(-1).tolist())]
    if pca is not None:
        p = flat("pca", pca, (views, 3), torch.float32)
        if not bool(torch.isfinite(p).all()) or bool((p.abs() > _FLT_MAX).any()):
            raise ValueError(f"{who}: pca: finite fp32 values")
        out.append(_host(C.c_float, p.reshape(-1).tolist()))
    return out


def _jitter_scratch(who, views, rows, cols, dev):
    if rows > 65535 or rows * cols > _JITTER_MAX_PIXELS:
        raise RuntimeError(f"{who}: views of {rows} x {cols}: at most 65535 rows and 2^24 pixels")
    nbytes = int(_lib.query("ecma_jitter_scratch_bytes", views, rows, cols))
    _need(nbytes > 0, lambda: f"{who}: no scratch size for {views} views of {rows} x {cols}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), C.c_longlong(nbytes)


def color_jitter(images_u8, factors, order, hue_shift):
    """torchvision's ColorJitter with given parameters on resident images: images_u8 uint8 [N,H,W,3] -> uint8 [N,H,W,3], Pillow's
    result byte for byte.  Per image: factors [N,3] (brightness, contrast, saturation; read where the operation is present), order
    [N,4] (codes 0 brightness, 1 contrast, 2 saturation, 3 hue in the order they run, then -1) and hue_shift [N] in 0..255, host
    values.  Each operation works on the uint8 result of the one before; contrast blends with the rounded mean gray of the image
    as it then stands.  Two launches where an image has contrast, else one; integer sums only: bit-reproducible."""
    who = "color_jitter"
    if not isinstance(images_u8, torch.Tensor):
        raise ValueError(f"{who}: images_u8 {type(images_u8).__name__}: a tensor")
    _on_device(images_u8)
    _need(images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[3] == 3 and images_u8.numel() > 0,
          lambda: f"{who}: images_u8 {images_u8.dtype} {tuple(images_u8.shape)}: want uint8 [N,H,W,3], none of them 0")
    N, H, W, _ = images_u8.shape
    fh, oh, hh = _jitter_views(who, N, factors, order, hue_shift)
    scratch, nbytes = _jitter_scratch(who, N, H, W, images_u8.device)
    src = images_u8.contiguous()
    out = torch.empty_like(src)
    _lib.call("ecma_color_jitter_fwd", _p(src), _p(out), N, H, W, fh, oh, hh, _p(scratch), nbytes, _stream())
    return out


def frame_prep_jitter(frames, crop_y0, crop_x0, th, tw, params, mean=FLYING3D_MEAN, std=FLYING3D_STD, want_image=False):
    """frame_prep's window decode of a packed shard with KITTI.transform's training augmentation in it (KITTI.py:144-191): frames
    = (rgb6 uint8 [B,H,W,6], disparity fp16|fp32 [B,H,W]), windows of th x tw at crop_y0/crop_x0, params a JitterParams of B
    samples (jitter_params) -> left, right [B,3,th,tw], disparity [B,th,tw] (and, with want_image, the left view clamped to 0..1
    as KITTI.py:189 returns it -- not frame_prep's raw 0..255 plane).  Per view: color_jitter's operations on the window, then in
    fp32 u / 255 + pca, clamp to 0..1, (x - mean) / std.  float32 [B,H,W,7] frames are not taken."""
    who = "frame_prep_jitter"
    if not isinstance(frames, (tuple, list)) or len(frames) != 2 or not all(isinstance(t, torch.Tensor) for t in frames):
        raise ValueError(f"{who}: frames: a packed shard (uint8 [B,H,W,6], fp16|fp32 [B,H,W])")
    if not isinstance(params, JitterParams):
        raise ValueError(f"{who}: params {type(params).__name__}: a JitterParams (jitter_params)")
    rgb, dsp, B, H, W = _packed_shard(who, frames)
    th, tw = _integer(who, "th", th, 1, None), _integer(who, "tw", tw, 1, None)
    ys, xs = _window_origins(who, crop_y0, crop_x0, B)
    if any(y < 0 or y + th > H for y in ys) or any(x < 0 or x + tw > W for x in xs):
        raise ValueError(f"{who}: windows of {th} x {tw} at {ys} / {xs}: inside the {H} x {W} frame")
    fields = dict(factors=(B, 2, 3), order=(B, 2, 4), hue_shift=(B, 2), pca=(B, 2, 3))
    for name, shape in fields.items():
        t = getattr(params, name)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{who}: params.{name}: a tensor of {shape} for {B} samples")
    fh, oh, hh, ph = _jitter_views(who, 2 * B, *(getattr(params, name).reshape((2 * B,) + shape[2:]) for name, shape in fields.items()))
    m3, s3 = _norm3(who, "mean", mean), _norm3(who, "std", std)
    scratch, nbytes = _jitter_scratch(who, 2 * B, th, tw, rgb.device)
    left, right, disp, image = _decode_outputs(B, th, tw, rgb.device, want_image)
    _lib.call("ecma_frame_prep_jitter_fwd", _p(rgb), _p(dsp), int(dsp.dtype == torch.float16), _p(left), _p(right), _p(disp), _p(image), B,
              H, W, _host(C.c_int, ys), _host(C.c_int, xs), th, tw, fh, oh, hh, ph, m3, s3, _p(scratch), nbytes, _stream())
    return _decoded(left, right, disp, image)


# ------------------------------------------------------------------------------------ stereo rectification
# DESIGN.md section 24; include/ecm_rectify.h.  The front of the chain: from a calibrated rig (K1, D1, K2, D2, R, T) and a raw,
# distorted pair to the normalised inputs of the network and the Q that disparity_reproject / point_cloud take.  stereo_rectify is
# host arithmetic in fp64 (Bouguet's construction); rectify_map is initUndistortRectifyMap in fp64 on the device, once per rig;
# remap_pair is the per-frame kernel: both views, bilinear, with frame_prep's normalisation, in one launch.  Forward only.
# The camera model is the pinhole with rational radial and tangential distortion; no fisheye, thin-prism or tilt terms.
Rectification = collections.namedtuple("Rectification", "R1 R2 P1 P2 Q size new_size")
_DIST_LENGTHS = (4, 5, 8)                     # k1 k2 p1 p2 [k3 [k4 k5 k6]]: OpenCV's order


def _calib(who, name, t, shape):
    """A calibration operand: a float64 CPU tensor of `shape` (None in it: any length) with finite entries, or ValueError."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.is_cuda or t.dim() != len(shape) \
            or any(s is not None and s != n for s, n in zip(shape, t.shape)):
        what = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name} {what}: a float64 CPU tensor {list(shape)}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{who}: {name} has a non-finite entry")
    return t.detach()


def _camera(who, name, K, D):
    """(fx, fy, cx, cy) and the eight coefficients k1 k2 p1 p2 k3 k4 k5 k6 (those not given: 0.0) as floats."""
    K, D = _calib(who, name, K, (3, 3)), _calib(who, "D" + name[1:], D, (None,))
    if D.shape[0] not in _DIST_LENGTHS:
        raise ValueError(f"{who}: D{name[1:]} holds {D.shape[0]} coefficients: one of {_DIST_LENGTHS} (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    k = K.tolist()
    if k[0][1] != 0 or k[1][0] != 0 or k[2] != [0.0, 0.0, 1.0] or not (k[0][0] > 0 and k[1][1] > 0):
        raise ValueError(f"{who}: {name} is not a pinhole matrix [fx 0 cx; 0 fy cy; 0 0 1] with fx, fy > 0")
    return (k[0][0], k[1][1], k[0][2], k[1][2]), D.tolist() + [0.0] * (8 - D.shape[0])


def _hw(who, name, size):
    if not isinstance(size, (tuple, list)) or len(size) != 2 or \
            any(not _is_int(v) or v < 1 for v in size):
        raise ValueError(f"{who}: {name} {size!r}: (H, W), two positive ints")
    return int(size[0]), int(size[1])


def _rotation_matrix(om):
    """Rodrigues: the rotation by |om| about om / |om| (float64 [3]); the zero vector gives the identity exactly."""
    theta = float(torch.linalg.vector_norm(om))
    eye = torch.eye(3, dtype=torch.float64)
    if theta == 0.0:
        return eye
    a = om / theta
    skew = torch.tensor([[0.0, -float(a[2]), float(a[1])], [float(a[2]), 0.0, -float(a[0])], [-float(a[1]), float(a[0]), 0.0]],
                        dtype=torch.float64)
    c, s = math.cos(theta), math.sin(theta)
    return c * eye + (1.0 - c) * torch.outer(a, a) + s * skew


def _rotation_vector(R):
    """Rodrigues' inverse: axis * angle of an orthonormal R (float64 [3,3]), the angle in [0, pi]."""
    v = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])            # 2 sin(angle) * axis
    s = float(torch.linalg.vector_norm(v)) / 2.0
    c = (float(R[0, 0] + R[1, 1] + R[2, 2]) - 1.0) / 2.0
    theta = math.atan2(s, c)
    if s > 1e-8:
        return v * (theta / (2.0 * s))
    if c > 0:
        return v / 2.0                                                                    # angle = sin(angle) to fp64 there
    sym = (R + R.T) / 2.0 + torch.eye(3, dtype=torch.float64)                             # near pi: 2 axis axis^T
    col = sym[:, int(torch.argmax(torch.diagonal(sym)))]
    axis = col / torch.linalg.vector_norm(col)
    if float(torch.dot(axis, v)) < 0:
        axis = -axis
    return axis * theta


def _align_to_x(t):
    """The smallest rotation taking t (float64 [3], non-zero) onto the x axis on the side t_x lies on (t_x = 0: the positive
    one): I + [v]x + [v]x^2 / (1 + c) with v = a x u, c = a . u for a = t / |t| and u = (+-1, 0, 0).  Exact identity where t is
    already on the axis."""
    a = t / torch.linalg.vector_norm(t)
    u = torch.tensor([-1.0 if float(t[0]) < 0 else 1.0, 0.0, 0.0], dtype=torch.float64)
    v = torch.linalg.cross(a, u)
    c = float(torch.dot(a, u))                                                            # >= 0
    skew = torch.tensor([[0.0, -float(v[2]), float(v[1])], [float(v[2]), 0.0, -float(v[0])], [-float(v[1]), float(v[0]), 0.0]],
                        dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + skew + (skew @ skew) / (1.0 + c)


def stereo_rectify(K1, D1, K2, D2, R, T, size, new_size=None, focal=None, center=None):
    """Bouguet's rectification of a horizontal rig, on the host in fp64: Rectification(R1, R2, P1, P2, Q, size, new_size).
    Conventions are OpenCV's: a point of the left camera frame is X2 = R X1 + T in the right one; K [3,3], D = k1 k2 p1 p2
    [k3 [k4 k5 k6]], R [3,3], T [3] are float64 CPU tensors; size and new_size (None: size) are (H, W).
    With r = R^(-1/2) (Rodrigues of minus half the rotation vector) and t = r T, wR is the smallest rotation taking t onto the x
    axis on the side of t_x; R1 = wR r^T and R2 = wR r rotate the left and the right camera frame into the common rectified
    frame, and R2 T = (t_x', 0, 0).  The intrinsics are this project's rule, not OpenCV's alpha / ROI logic: f = focal, or
    min(K1[1,1], K2[1,1]) * new_H / H; (cx, cy) = center, or the mean of the two principal points scaled by new_W / W and
    new_H / H; both views share them (zero disparity at infinity).  P1 = [f 0 cx 0; 0 f cy 0; 0 0 1 0], P2 the same with
    P2[0,3] = f t_x', Q = q_matrix(f, |t_x'|, cx, cy).  ValueError: wrong shapes or dtypes, non-finite entries, len(D) not 4, 5
    or 8, R not orthonormal to 1e-6, T = 0, a vertical rig (|t_y| > |t_x|), and t_x' > 0 (the "right" camera lies on the left:
    swap the views)."""
    who = "stereo_rectify"
    (_, fy1, cx1, cy1), _ = _camera(who, "K1", K1, D1)
    (_, fy2, cx2, cy2), _ = _camera(who, "K2", K2, D2)
    R, T = _calib(who, "R", R, (3, 3)), _calib(who, "T", T, (3,))
    H, W = _hw(who, "size", size)
    Hn, Wn = (H, W) if new_size is None else _hw(who, "new_size", new_size)
    if focal is not None and not _is_real(focal, "> 0"):
        raise ValueError(f"{who}: focal {focal!r}: None or a finite number > 0")
    if center is not None and (not isinstance(center, (tuple, list)) or len(center) != 2 or not all(_is_real(v) for v in center)):
        raise ValueError(f"{who}: center {center!r}: None or (cx, cy), two finite numbers")
    eye = torch.eye(3, dtype=torch.float64)
    if float((R @ R.T - eye).abs().max()) > 1e-6 or float(torch.linalg.det(R)) < 0:
        raise ValueError(f"{who}: R is not a rotation (R R^T = I to 1e-6, det +1)")
    if float(torch.linalg.vector_norm(T)) == 0.0:
        raise ValueError(f"{who}: T is zero: no baseline")
    r = _rotation_matrix(-0.5 * _rotation_vector(R))
    t = r @ T
    if abs(float(t[1])) > abs(float(t[0])):
        raise ValueError(f"{who}: a vertical rig (|t_y| {abs(float(t[1]))!r} > |t_x| {abs(float(t[0]))!r}): only horizontal rigs")
    if float(t[0]) > 0:
        raise ValueError(f"{who}: t_x' > 0: the \"right\" camera lies on the left of the \"left\" one; swap the views")
    wR = _align_to_x(t)
    R1, R2 = wR @ r.T, wR @ r
    tx = float((R2 @ T)[0])
    sy, sx = Hn / H, Wn / W                                                               # 1.0 exactly where new_size is size
    f = float(focal) if focal is not None else min(fy1, fy2) * sy
    cx, cy = (float(center[0]), float(center[1])) if center is not None else ((cx1 + cx2) / 2.0 * sx, (cy1 + cy2) / 2.0 * sy)
    P1 = torch.tensor([[f, 0.0, cx, 0.0], [0.0, f, cy, 0.0], [0.0, 0.0, 1.0, 0.0]], dtype=torch.float64)
    P2 = P1.clone()
    P2[0, 3] = f * tx
    return Rectification(R1, R2, P1, P2, q_matrix(f, abs(tx), cx, cy), (H, W), (Hn, Wn))


def rectify_tile_width():
    """The output columns one workgroup of rectify_map and remap_pair covers (a size query of the library: no GPU needed)."""
    return int(_lib.query("ecmr_tile_width"))


def rectify_map_params(K, D, R, P):
    """The doubles rectify_map hands to the device, as a float64 CPU tensor: iR = (P[:, :3] R)^-1 row-major (taken here, on the
    host), fx fy cx cy of K, then k1 k2 p1 p2 k3 k4 k5 k6 (coefficients D does not give: 0).  ValueError for operands that are not
    float64 CPU tensors K [3,3], D [4|5|8], R [3,3], P [3,4] with finite entries, and for a singular P[:, :3] R."""
    who = "rectify_map"
    cam, dist = _camera(who, "K", K, D)
    R, P = _calib(who, "R", R, (3, 3)), _calib(who, "P", P, (3, 4))
    M = P[:, :3] @ R
    if not abs(float(torch.linalg.det(M))) > 1e-12 * float(M.abs().max()) ** 3:
        raise ValueError(f"{who}: P[:, :3] R is singular")
    iR = torch.linalg.inv(M)
    if not bool(torch.isfinite(iR).all()):
        raise ValueError(f"{who}: P[:, :3] R is singular")
    params = torch.cat([iR.reshape(9), torch.tensor(list(cam) + dist, dtype=torch.float64)])
    _need(params.numel() == _lib.query("ecmr_rectify_map_params"), "rectify_map: the library expects another parameter count")
    return params


@torch.no_grad()
def rectify_map(K, D, R, P, new_size, device):
    """initUndistortRectifyMap on the device, in fp64, one launch: map [2,Ho,Wo] fp32 for new_size = (Ho, Wo), plane 0 the source
    x and plane 1 the source y of every rectified pixel, each rounded once to fp32.  K, D: the camera; R: its rectifying
    rotation (R1 or R2 of stereo_rectify); P: its new projection (P1 or P2; the fourth column is not used).  The operation
    order is written out in include/ecm_rectify.h."""
    params = rectify_map_params(K, D, R, P)
    Ho, Wo = _hw("rectify_map", "new_size", new_size)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("ecm ops run only on the MI355X HIP path: got a CPU device (no CPU fallback exists)")
    with torch.cuda.device(device):
        pd = params.to(device)
        out = torch.empty(2, Ho, Wo, device=device, dtype=torch.float32)
        # Ho * Wo >= 2^31 is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
        _lib.call("ecmr_rectify_map_fwd", _p(pd), _p(out), Ho, Wo, _stream())
    return out


@torch.no_grad()
def remap_pair(left_raw, right_raw, map_left, map_right, mean=FLYING3D_MEAN, std=FLYING3D_STD, border=0.0, want_image=False,
               with_mask=False):
    """The raw pair through its rectification maps to the network's inputs, both views in one launch: (left, right), each
    [B,3,Ho,Wo] fp32 = (s / 255 - mean) / std with s the bilinear sample of the raw frame at the map's coordinates -- frame_prep's
    arithmetic, so a map of integer coordinates reproduces its planes bit for bit.  left_raw, right_raw: uint8 [B,H,W,3] or
    float32 [B,3,H,W] holding 0..255; map_left, map_right: fp32 [2,Ho,Wo] (one rig) or [B,2,Ho,Wo] (rectify_map builds them).  A
    tap outside the source is `border` (0..255 units); a non-finite map entry gives border in every channel.  want_image=True
    adds the rectified left image in /255 units (the colours of a point cloud); with_mask=True adds (mask_left, mask_right), bool
    [B,Ho,Wo]: True where the coordinates are finite and all four taps lie inside the source.  Returns
    (left, right[, image][, mask_left, mask_right]).  No atomics: bit-reproducible.  What bilinear resampling does to EPE or D1 is
    not measured."""
    who = "remap_pair"
    for t in (left_raw, right_raw, map_left, map_right):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(_CPU_TENSOR)
    u8 = left_raw.dtype == torch.uint8
    _need(left_raw.dim() == 4 and ((u8 and left_raw.shape[3] == 3) or (left_raw.dtype == torch.float32 and left_raw.shape[1] == 3))
          and left_raw.numel() > 0,
          lambda: f"{who}: left_raw {left_raw.dtype} {tuple(left_raw.shape)}: want uint8 [B,H,W,3] or float32 [B,3,H,W]")
    _need(right_raw.dtype == left_raw.dtype and right_raw.shape == left_raw.shape,
          lambda: f"{who}: right_raw {right_raw.dtype} {tuple(right_raw.shape)} against left_raw {left_raw.dtype} {tuple(left_raw.shape)}")
    B, H, W = (left_raw.shape[0], left_raw.shape[1], left_raw.shape[2]) if u8 else (left_raw.shape[0], left_raw.shape[2], left_raw.shape[3])
    _need(map_left.dtype == torch.float32 and map_left.dim() in (3, 4) and map_left.shape[-3] == 2 and map_left.numel() > 0
          and (map_left.dim() == 3 or map_left.shape[0] == B),
          lambda: f"{who}: map_left {map_left.dtype} {tuple(map_left.shape)}: want float32 [2,Ho,Wo] or [{B},2,Ho,Wo]")
    _need(map_right.dtype == torch.float32 and map_right.shape == map_left.shape,
          lambda: f"{who}: map_right {map_right.dtype} {tuple(map_right.shape)} against map_left {tuple(map_left.shape)}")
    m3, s3 = _norm3(who, "mean", mean), _norm3(who, "std", std, nonzero=True)
    _real(who, "border", border, fp32=True)
    Ho, Wo = map_left.shape[-2:]
    lr, rr, ml, mr = left_raw.detach().contiguous(), right_raw.detach().contiguous(), _c(map_left.detach()), _c(map_right.detach())
    left, right, _, image = _decode_outputs(B, Ho, Wo, lr.device, want_image, with_disp=False)
    mask_l = torch.empty(B, Ho, Wo, device=lr.device, dtype=torch.uint8) if with_mask else None
    mask_r = torch.empty_like(mask_l) if with_mask else None
    # B * max(H * W, Ho * Wo) >= 2^31 is refused by the library before any launch (ECM_EUNSUP -> RuntimeError)
    _lib.call("ecmr_remap_pair_fwd", _p(lr), _p(rr), int(u8), _p(ml), _p(mr), int(map_left.dim() == 4), _p(left), _p(right),
              _p(image), _p(mask_l), _p(mask_r), B, H, W, Ho, Wo, m3, s3, float(border), _stream())
    out = (left, right) + ((image,) if want_image else ())
    return out + ((mask_l.view(torch.bool), mask_r.view(torch.bool)) if with_mask else ())


def _out_row(out, n, device):
    """The `out=` operand of the evaluation ops: None -> a fresh float32[n] on `device`; else a contiguous fp32 view of n floats
    there (e.g. a row of a preallocated [n_batches, n] log) that the kernel writes in place."""
    if out is None:
        return torch.empty(n, device=device, dtype=torch.float32)
    _chk(out)
    _need(out.numel() == n and out.is_contiguous() and out.device == device,
          lambda: f"out: want a contiguous float32 view of {n} elements on {device}, got {tuple(out.shape)} "
                  f"(strides {out.stride()}) on {out.device}")
    return out


def eval_epe(pred, gt, crop_h=540, crop_w=960, maxdisp=192, out=None):
    """SceneFlow evaluation of test.py:69-94 on the device: pred [B,1,Hp,Wp] or [B,Hp,Wp] (output3), gt [B,Hg,Wg];
    -> float32[6] = (epe, epe_non, epe_true, n, n_non, n_true), both tensors cropped to [:crop_h, :crop_w].
    out: a contiguous float32 device view of 6 elements to write instead (a row of a log); it is returned."""
    _chk(pred, gt)
    if pred.dim() == 4:
        pred = pred.squeeze(1)
    pred, gt = _c(pred), _c(gt)
    B, Hp, Wp = pred.shape
    Bg, Hg, Wg = gt.shape
    if B != Bg:
        raise RuntimeError(f"prediction / ground-truth batch sizes differ: {B} vs {Bg}")
    out = _out_row(out, 6, pred.device)
    n = B * int(crop_h) * int(crop_w)
    _call_scratch(pred.device, "ecm_eval_epe_scratch_bytes", (C.c_longlong(n),), "ecm_eval_epe", _p(pred), _p(gt), _p(out),
                  _SCRATCH, B, Hp, Wp, Hg, Wg, int(crop_h), int(crop_w), float(maxdisp), _stream())
    return out


def eval_kitti(pred, gt, maxdisp=192, out=None, per_sample=False):
    """KITTI validation of eval_kitti.py:84-103 on the device, whole frame, no crop: pred [B,1,H,W] or [B,H,W] (output3),
    gt [B,H,W] -> float32[8] = (loss, loss_non, loss_true, loss_3, n_mask, n_non, n_true, n_good) with mask = 0 < gt < maxdisp,
    mask_non = mask_true = mask and x - gt >= 0 (identical in the reference), loss_3 the 3-px / 5 % error rate in percent.
    An empty mask gives NaN.  per_sample=True: -> (row, table [B,8]) with the same columns for each image alone.
    out: a contiguous float32 device view of 8 elements to write instead (a row of a [n_batches, 8] log); it is returned.
    Nothing here synchronises with the host."""
    _chk(pred, gt)
    if pred.dim() == 4:
        _need(pred.shape[1] == 1, lambda: f"eval_kitti: pred {tuple(pred.shape)}: want [B,1,H,W] or [B,H,W]")
        pred = pred.squeeze(1)
    _need(pred.dim() == 3 and pred.shape == gt.shape and pred.numel() > 0,
          lambda: f"eval_kitti: pred {tuple(pred.shape)} / gt {tuple(gt.shape)}: want the same non-empty [B,H,W]")
    pred, gt = pred.contiguous(), gt.contiguous()        # any 4-byte alignment: the kernel picks its load width, the row is the same
    B, H, W = pred.shape
    out = _out_row(out, 8, pred.device)
    table = torch.empty(B, 8, device=pred.device, dtype=torch.float32) if per_sample else None
    _call_scratch(pred.device, "ecm_eval_kitti_scratch_bytes", (B, H, W), "ecm_eval_kitti", _p(pred), _p(gt), _p(out), _p(table),
                  _SCRATCH, B, H, W, float(maxdisp), _stream())
    return (out, table) if per_sample else out


# DESIGN.md section 22.  What eval_sparsification returns: the curves of the K measures (epe in pixels, d1 in percent, each
# [B,K,steps]) and of the oracle ([B,steps]) -- views of one table -- the areas between them ([B,K]: ause against the oracle, aurg
# against random removal, whose curve is flat at the first point) and count [B,3] int64 = (n, E_tot, bad_tot).
Sparsification = collections.namedtuple("Sparsification", "epe d1 oracle_epe oracle_d1 ause_epe ause_d1 aurg_epe aurg_d1 count")


def eval_sparsification_limits():
    """(the most measures, the most steps) eval_sparsification takes (size queries of the library: no GPU needed)."""
    return int(_lib.query("ecm_eval_sparsify_max_measures")), int(_lib.query("ecm_eval_sparsify_max_steps"))


def check_sparsification_parameters(n_measures, steps, maxdisp=192, who="eval_sparsification"):
    """(steps, maxdisp): an int in 1..64 and a finite number > 0, with 1..8 measures."""
    max_k, max_steps = eval_sparsification_limits()
    if not 1 <= n_measures <= max_k:
        raise ValueError(f"{who}: {n_measures} measures: 1..{max_k}")
    return _integer(who, "steps", steps, 1, max_steps), _real(who, "maxdisp", maxdisp, "> 0")


def sparsification_areas(curve, oracle):
    """(ause, aurg) of curves [..., K, steps] against oracle [..., steps], in fp64: ause = mean_j(curve_j - oracle_j), the area
    between a measure and the best possible ranking; aurg = mean_j(curve_0 - curve_j), the area random removal leaves above it."""
    curve, oracle = curve.double(), oracle.double()
    return (curve - oracle.unsqueeze(-2)).mean(-1), (curve[..., :1] - curve).mean(-1)


@torch.no_grad()
def eval_sparsification(pred, gt, measures, maxdisp=192, steps=20):
    """Sparsification curves on the device: pred [B,1,H,W] or [B,H,W], gt [B,H,W], measures a sequence of 1..8 planes of pred's
    shape in which a HIGHER value means LESS trusted (negate a confidence).  Per sample, over the pixels with 0 < gt < maxdisp: for
    j = 0..steps-1 the r_j = floor(j n / steps) least trusted pixels are removed -- equal values leave pro rata, NaN first, -0.0 as
    +0.0 -- and the mean |pred - gt| (epe) and the 3-px / 5 % error rate in percent (d1, eval_kitti's) of the rest are recorded;
    the oracle removes the largest errors first (its d1: the bad pixels first).  -> Sparsification.  Errors enter the sums as
    integers, rintf(min(e, 4095) * 65536): every mean is within 2^-17 px of the exact one, errors above 4095 px (and NaN) count as
    4095, and the result is bit-reproducible and the same whatever else is in the batch.  Exact on the full 32-bit value of a
    measure: a radix selection of the `steps` cut ranks, not a sort.  A sample without valid pixels gives NaN rows.  The areas
    are formed in fp64 from the table by torch ops and cast to fp32.  Nothing here synchronises with the host.
    Limits: H * W < 2^31, B <= 65535, 1..8 measures, steps in 1..64."""
    measures = list(measures)
    steps, maxdisp = check_sparsification_parameters(len(measures), steps, maxdisp)         # before any device work
    _chk(pred, gt, *measures)
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    _need(pred.dim() == 3 and pred.shape == gt.shape and pred.numel() > 0,
          lambda: f"eval_sparsification: pred {tuple(pred.shape)} / gt {tuple(gt.shape)}: want the same non-empty [B,H,W]")
    B, H, W = pred.shape
    planes = []
    for k, m in enumerate(measures):
        if m.dim() == 4 and m.shape[1] == 1:
            m = m[:, 0]
        _need(m.shape == pred.shape, lambda: f"eval_sparsification: measure {k} {tuple(m.shape)} against pred {tuple(pred.shape)}")
        planes.append(m.detach().contiguous())
    if H * W >= 1 << 31 or B > 65535:
        raise ValueError(f"eval_sparsification: {B} x {H} x {W}: H * W < 2^31 and B <= 65535")
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()      # any 4-byte alignment: the kernel picks its load width
    K = len(planes)
    table = torch.empty(B, K + 1, steps, 2, device=pred.device, dtype=torch.float32)
    count = torch.empty(B, 3, device=pred.device, dtype=torch.int64)
    ptrs = _host(C.c_void_p, (m.data_ptr() for m in planes))
    _call_scratch(pred.device, "ecm_eval_sparsify_scratch_bytes", (B, H, W, K, steps), "ecm_eval_sparsify", _p(pred), _p(gt), ptrs,
                  _p(table), _p(count), _SCRATCH, B, H, W, K, steps, float(maxdisp), _stream())
    epe, d1, oracle_epe, oracle_d1 = table[:, :K, :, 0], table[:, :K, :, 1], table[:, K, :, 0], table[:, K, :, 1]
    ause_epe, aurg_epe = sparsification_areas(epe, oracle_epe)
    ause_d1, aurg_d1 = sparsification_areas(d1, oracle_d1)
    return Sparsification(epe, d1, oracle_epe, oracle_d1, ause_epe.float(), ause_d1.float(), aurg_epe.float(), aurg_d1.float(), count)


def disparity_to_uint16(pred, h, w, scale=256.0):
    """KITTI submission image of test_kitti.py:163-168: pred [B,1,Hp,Wp] or [B,Hp,Wp] (output3) -> uint16 [B,max h,max w]
    with out[b,:h[b],:w[b]] = (pred[b,-h[b]:,-w[b]:] * scale).astype(uint16) (numpy cast semantics), zeros elsewhere.
    h, w: per-sample original sizes (ints or sequences)."""
    _chk(pred)
    if pred.dim() == 4:
        pred = pred.squeeze(1)
    pred = _c(pred)
    B, Hp, Wp = pred.shape
    hs = [int(h)] * B if isinstance(h, int) else [int(v) for v in h]
    ws = [int(w)] * B if isinstance(w, int) else [int(v) for v in w]
    Ho, Wo = max(hs), max(ws)
    out = torch.empty(B, Ho, Wo, device=pred.device, dtype=torch.uint16)
    _lib.call("ecm_disp_to_u16", _p(pred), _p(out), B, Hp, Wp, _host(C.c_int, hs), _host(C.c_int, ws), Ho, Wo,
              float(scale), _stream())
    return out


class StereoLoss3(torch.autograd.Function):
    """Loss of the training scripts and the KITTI validation metrics in one pass (train.py:162,172-174;
    train_kitti.py:205-216).  Returns (loss, metrics[8]); metrics = [loss, #mask, epe, err3 %, m1, m2, m3, 0] (no grad)."""

    @staticmethod
    def forward(ctx, p1, p2, p3, gt, maxdisp, w1, w2, w3):
        _chk(p1, p2, p3, gt)
        if not (p1.numel() == p2.numel() == p3.numel() == gt.numel()):
            raise RuntimeError(f"prediction / ground-truth sizes differ: {tuple(p1.shape)} {tuple(p2.shape)} "
                               f"{tuple(p3.shape)} vs {tuple(gt.shape)}")
        p1, p2, p3, gt = _c(p1), _c(p2), _c(p3), _c(gt)
        n = gt.numel()
        out = torch.empty(8, device=gt.device, dtype=gt.dtype)
        _call_scratch(gt.device, "ecm_stereo_loss_scratch_bytes", (C.c_longlong(n),), "ecm_stereo_loss_fwd",
                      _p(p1), _p(p2), _p(p3), _p(gt), _p(out), _SCRATCH, C.c_longlong(n), float(maxdisp), float(w1),
                      float(w2), float(w3), _stream())
        ctx.save_for_backward(p1, p2, p3, gt, out)
        ctx.cfg = (float(maxdisp), float(w1), float(w2), float(w3))
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gloss, _gmetrics):
        p1, p2, p3, gt, out = ctx.saved_tensors
        maxdisp, w1, w2, w3 = ctx.cfg
        gloss = _c(gloss.reshape(1).to(gt.dtype))
        g1, g2, g3 = _empty_like(p1), _empty_like(p2), _empty_like(p3)
        _lib.call("ecm_stereo_loss_bwd", _p(p1), _p(p2), _p(p3), _p(gt), _p(out), _p(gloss), _p(g1), _p(g2), _p(g3),
                  C.c_longlong(gt.numel()), float(maxdisp), float(w1), float(w2), float(w3), _stream())
        return g1, g2, g3, None, None, None, None, None


def stereo_loss3(preds, gt, maxdisp=192, weights=(0.5, 0.7, 1.0)):
    """-> (loss, metrics[8]) for the three predictions of a model (each [B,1,H,W] or [B,H,W]) and gt [B,H,W]."""
    p1, p2, p3 = preds
    return StereoLoss3.apply(p1, p2, p3, gt, float(maxdisp), *map(float, weights))


def group_norm_act(x, gamma, beta, skip=None, relu=False, head=0, out_dtype=None):
    """head > 0: returns (y, x[:head]) -- see GroupNormAct.forward.  A bf16 x, or out_dtype=torch.bfloat16 (the boundary into
    the bf16 region: fp32 x), runs the bf16 inference kernels and returns a bf16 y (see aggregation_dtype)."""
    if x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16:
        _need(not head, "group_norm_act: the bf16 form takes no head fork")
        _bf16_region(_AGG, _ENC, _DEC).no_grad("group_norm_act")
        return _gn_apply_two_stage(x, gamma, beta, skip, bool(relu), torch.bfloat16)
    _need(out_dtype in (None, torch.float32), lambda: f"group_norm_act: out_dtype {out_dtype}: float32 or bfloat16")
    _need(0 <= int(head) <= x.shape[0], lambda: f"group_norm_act: head {head} of a batch of {x.shape[0]}")
    if head and not (torch.is_grad_enabled() and x.requires_grad):
        return GroupNormAct.apply(x, gamma, beta, skip, bool(relu), 0), x[:head]
    return GroupNormAct.apply(x, gamma, beta, skip, bool(relu), int(head))


def gn_cluster_mode(mode=-1):
    """Process-wide switch of the one-pass GroupNorm kernels (include/ecm_hip.h: ecm_gn3d_cluster_mode): 1 = cluster kernels
    (default), 0 = two-stage kernels only -- the choice when several processes share one device; returns the previous mode."""
    return _lib.query("ecm_gn3d_cluster_mode", int(mode))


def check_async_errors(clear=True):
    """Synchronise the current device and raise if a cluster kernel's bounded wait expired since the last check (its
    outputs are NaN).  Call once per step (bench.py and the tests do); every later GroupNorm call raises on its own too."""
    torch.cuda.synchronize()
    rc = _lib.query("ecm_async_status", 1 if clear else 0)
    if rc != 0:
        _GN_CLUSTER.clear()                    # a timed-out cluster leaves the exchange memory in an unknown state
        msg = _lib.load().ecm_error_string(rc)
        raise RuntimeError(f"asynchronous device-side failure ({rc}): {msg.decode() if msg else '?'}")


# ---- opt-in bf16 inference of the 3-D aggregation stack ----------------------------------------------------------------------
# Inside `with aggregation_dtype(torch.bfloat16):` the models run dres0's second convolution through the classifiers' 32 -> 1
# layers on bf16 volumes (csrc/bf16_infer.hip on the body of csrc/bf16_conv3d.h: bf16 operands on the matrix cores, fp32
# accumulation, one rounding per output).
# The setting is process-wide like WINOGRAD (nn.DataParallel replicas run in other threads), inference only (nothing here has
# a backward: a 3-D op reached with grad enabled raises), and the fp32 path outside the block is untouched.  The ops below
# dispatch on the dtype of the volume; weights stay fp32 parameters, packed to bf16 images per call (cached under
# frozen_weights() beside the fp32 layouts, under their own keys).
class _Bf16Switch:
    """A process-wide opt-in bf16 inference switch (aggregation_dtype, encoder_dtype, decoder_dtype): nests, restores the previous setting
    on exit, and is inference only."""

    def __init__(self, name, what):
        self.name, self.what, self.dtype = name, what, torch.float32

    @_contextlib.contextmanager
    def scope(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{self.name}: {dtype} is not supported (torch.float32 or torch.bfloat16)")
        prev, self.dtype = self.dtype, dtype
        try:
            yield
        finally:
            self.dtype = prev

    def on(self):
        return self.dtype == torch.bfloat16

    def no_grad(self, op):
        """Raise the inference-only error if grad is enabled."""
        if torch.is_grad_enabled():
            raise RuntimeError(f"{op}: {self.what} has no backward (inference only); run the model under torch.no_grad() "
                               f"or leave the {self.name}(torch.bfloat16) block")

    def guard(self, op):
        """An op reached inside a bf16 block with grad enabled raises before it launches anything (no silent fp32 path)."""
        if self.on():
            self.no_grad(op)


_AGG = _Bf16Switch("aggregation_dtype", "bf16 aggregation")


def _bf16_region(*switches):
    """The switch whose block an op shared by several bf16 regions was reached in (for its error text): the first one that is
    on, else the first."""
    return next((s for s in switches if s.on()), switches[0])


def aggregation_dtype(dtype):
    """torch.float32 (the default; a no-op) or torch.bfloat16 for the 3-D aggregation stack inside the block; nests and
    restores the previous setting on exit.  bf16 is inference only: run the model under torch.no_grad()."""
    return _AGG.scope(dtype)


def aggregation_bf16():
    """True inside an aggregation_dtype(torch.bfloat16) block."""
    return _AGG.on()


def _chk_bf16(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.bfloat16):
            raise RuntimeError(f"ecm bf16 ops take bfloat16 CUDA volumes (got {t.dtype} on {t.device})")


# the two families of csrc/bf16_conv3d.h: (size query, pack entry) and the stem of their frozen_weights() cache keys
_BF16_PACK = (("ecm_conv3d_bf16_packed_elems", "ecm_conv3d_bf16_pack_weight"), "bf16")
_SPLIT_PACK = (("ecm_conv3d_split_packed_elems", "ecm_conv3d_split_pack_weight"), "split")


def _pack_taps(w, transposed, entries, stem):
    """bf16 weight image [Ci/8][terms][28][Co][8] of a 3x3x3 weight read as a convolution (w [Co,Ci,27]) or, transposed, as a
    transposed convolution (w [Ci,Co,27]): one term for _BF16_PACK, the three split terms for _SPLIT_PACK -- the operands
    _pack_conv(w) and _pack_deconv(w) build for the fp32 kernels."""
    Ci, Co = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    elems, pack = entries

    def build():
        wc = _c(w.detach())
        packed = torch.empty(_lib.query(elems, Ci, Co), device=w.device, dtype=torch.bfloat16)
        _lib.call(pack, _p(wc), _p(packed), Ci, Co, int(transposed), _stream())
        return packed
    return _cached_pack(w, stem + ("_deconv" if transposed else "_conv"), build)


def _pack_bf16(w, transposed):
    return _pack_taps(w, transposed, *_BF16_PACK)


def _pack_split(w, transposed):
    return _pack_taps(w, transposed, *_SPLIT_PACK)


def _conv3d_bf16(x, w, stride, fork):
    _AGG.no_grad("conv3d_k3")
    _chk_bf16(x)
    _chk(w)
    _need(x.dim() == 5 and w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and w.shape[1] == x.shape[1] and stride in (1, 2)
          and x.shape[1] in (32, 64) and w.shape[0] in (32, 64) and x.numel() > 0,
          lambda: f"conv3d_k3 (bf16): x {tuple(x.shape)}, w {tuple(w.shape)}, stride {stride}: want [B,Ci,D,H,W], [Co,Ci,3,3,3] "
                  "with Ci, Co in {32, 64}, stride 1|2")
    x = _c(x)
    B, Ci, D, H, W = x.shape
    Co = w.shape[0]
    y = torch.empty(B, Co, (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1, device=x.device,
                    dtype=torch.bfloat16)
    _lib.call("ecm_conv3d_k3_bf16_fwd", _p(x), _p(_pack_bf16(w, False)), _p(y), B, Ci, Co, D, H, W, stride, _stream())
    return (y, x) if fork else y


def _deconv3d_bf16(x, w):
    _AGG.no_grad("deconv3d_k3s2")
    _chk_bf16(x)
    _chk(w)
    _need(x.dim() == 5 and w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and w.shape[0] == x.shape[1]
          and x.shape[1] in (32, 64) and w.shape[1] in (32, 64) and x.numel() > 0,
          lambda: f"deconv3d_k3s2 (bf16): x {tuple(x.shape)}, w {tuple(w.shape)}: want [B,Ci,D,H,W] and ConvTranspose3d's "
                  "[Ci,Co,3,3,3] with Ci, Co in {32, 64}")
    x = _c(x)
    B, Ci, D, H, W = x.shape
    Co = w.shape[1]
    y = torch.empty(B, Co, 2 * D, 2 * H, 2 * W, device=x.device, dtype=torch.bfloat16)
    _lib.call("ecm_deconv3d_k3s2_bf16_fwd", _p(x), _p(_pack_bf16(w, True)), _p(y), B, Ci, Co, D, H, W, _stream())
    return y


# ---- opt-in split-bf16 products for the stride-2 3-D convolutions ------------------------------------------------------------
# Inside `with split_products("bf16x3"):` the stride-2 family (the hourglass's conv1/conv3 and its two transposed
# convolutions, cmfsm.py:244-281) runs csrc/split_bf16.hip (the same body, csrc/bf16_conv3d.h): every fp32 operand is split
# into three bf16 terms and the six leading cross products accumulate in fp32 on the bf16 matrix cores.  Tensors stay fp32, the
# result is fp32-equivalent (the
# fp64 yardstick of the fp32 kernels, tests/test_hip_split_bf16_fp64.py) and the autograd Functions are the usual ones, so the
# block works with grad enabled -- unlike the bf16 regions above, which change the numerics and are inference only.
# The setting is process-wide like WINOGRAD, nests and restores.  It is read when a layer's FORWARD runs and rides on the
# autograd node, so a backward pass started after the block has closed still takes the data-gradient kernels the forward chose.
# What does not fit the split kernels keeps the fp32 kernels without an error: stride 1, channel counts outside {32, 64}, volumes
# whose byte offsets pass 2^31, and a kind that is not selected.  That fallback is not a quiet change of numerics: both paths
# meet the same bound.  Weight gradients always stay on the fp32 kernels; bf16 volumes still take the bf16 path.
# Packed split weights are cached under frozen_weights() like every other layout (keys "split_conv" / "split_deconv").
SPLIT_MODES = ("fp32", "bf16x3")
# the kinds `split_products("bf16x3")` turns on when none are named; a kind measured slower than its fp32 kernel at the bench
# geometry is left out (tools/split_bf16_time.py, profiles/r10_split_bf16_time.json)
SPLIT_ALL_KINDS = frozenset({"conv_fwd", "conv_dgrad", "deconv_fwd", "deconv_dgrad"})
# As measured in round 10 NO kind is faster than its fp32 kernel over the two layers it serves (0.68-0.81x on the 32 <-> 64 level,
# 0.74-1.20x on the 64 -> 64 level), so the default set is empty and `split_products("bf16x3")` changes nothing until kinds are named.
SPLIT_DEFAULT_KINDS = frozenset()
_SPLIT_MODE = "bf16x3" if _os.environ.get("ECM_SPLIT_BF16", "0") == "1" else "fp32"
_SPLIT_KINDS = SPLIT_DEFAULT_KINDS


@_contextlib.contextmanager
def split_products(mode, kinds=None):
    """"fp32" (the default; a no-op) or "bf16x3": inside the block the stride-2 3-D convolutions of fp32 volumes run the
    split-bf16 kernels, forward and data gradient, with or without grad.  kinds: which of SPLIT_ALL_KINDS to turn on
    (default SPLIT_DEFAULT_KINDS, which holds the kinds measured faster than fp32 -- none so far).  Nests and restores the previous setting on exit; ECM_SPLIT_BF16=1 makes "bf16x3" the
    process default."""
    global _SPLIT_MODE, _SPLIT_KINDS
    if mode not in SPLIT_MODES:
        raise ValueError(f"split_products: {mode!r} is not supported (one of {SPLIT_MODES})")
    kinds = SPLIT_DEFAULT_KINDS if kinds is None else frozenset(kinds)
    if not kinds <= SPLIT_ALL_KINDS:
        raise ValueError(f"split_products: unknown kinds {sorted(kinds - SPLIT_ALL_KINDS)} (of {sorted(SPLIT_ALL_KINDS)})")
    prev = (_SPLIT_MODE, _SPLIT_KINDS)
    _SPLIT_MODE, _SPLIT_KINDS = mode, kinds
    try:
        yield
    finally:
        _SPLIT_MODE, _SPLIT_KINDS = prev


def split_products_on():
    """True inside a split_products("bf16x3") block (or under ECM_SPLIT_BF16=1 outside any block)."""
    return _SPLIT_MODE == "bf16x3"


def split_supported(Ci, Co, big_voxels):
    """Do the split kernels take this layer?  Ci, Co: the kernel's input and output channels; big_voxels: D*H*W of the larger
    of its two volumes (byte offsets inside one sample must stay below 2^31)."""
    return Ci in (32, 64) and Co in (32, 64) and max(Ci, Co) * int(big_voxels) * 4 < 0x7fffffff


def _split_use(kind, x, Ci, Co):
    """Does this launch take the split kernel?  x: the layer's forward input (the small grid of a transposed convolution)."""
    if _SPLIT_MODE != "bf16x3" or kind not in _SPLIT_KINDS or x.dtype != torch.float32:
        return False
    vox = x.shape[2] * x.shape[3] * x.shape[4]
    return split_supported(Ci, Co, vox * 8 if kind.startswith("deconv") else vox)


def _split_conv_fwd(x, packed, Co):
    B, Ci, D, H, W = x.shape
    y = torch.empty(B, Co, (D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device, dtype=x.dtype)
    _lib.call("ecm_conv3d_k3s2_split_fwd", _p(x), _p(packed), _p(y), B, Ci, Co, D, H, W, _stream())
    return y


def _split_deconv_fwd(x, packed, Co, out_dhw):
    B, Ci, D, H, W = x.shape
    Do, Ho, Wo = out_dhw
    y = torch.empty(B, Co, Do, Ho, Wo, device=x.device, dtype=x.dtype)
    _lib.call("ecm_deconv3d_k3s2_split_fwd", _p(x), _p(packed), _p(y), B, Ci, Co, D, H, W, Do, Ho, Wo, _stream())
    return y


def _gn_stats(x):
    """GroupNorm(32) statistics [B,32,2] (mean, rstd) of an fp32 or bf16 volume (two-stage kernels)."""
    B, Cc = x.shape[:2]
    S = x.numel() // (B * Cc)
    stats = torch.empty(B, GN_GROUPS, 2, device=x.device, dtype=torch.float32)
    name = "ecm_gn3d_stats_bf16" if x.dtype == torch.bfloat16 else "ecm_gn3d_stats"
    _call_scratch(x.device, "ecm_gn3d_scratch_bytes", (B, Cc, C.c_longlong(S)), name, _p(x), _p(stats), _SCRATCH,
                  B, Cc, C.c_longlong(S), float(GN_EPS), _stream(), call=_gn_call)
    return stats


def _gn_apply_two_stage(x, gamma, beta, skip, relu, out):
    """relu?(GroupNorm32(x)*gamma+beta (+ skip)) by the two-stage kernels for the bf16 paths.  x fp32 or bf16, skip bf16;
    out: torch.bfloat16 (a bf16 y), torch.float32 (a bf16 x written in fp32) or "dual" (bf16 x: fp32 y and its bf16 copy)."""
    x_bf16 = x.dtype == torch.bfloat16
    what = "group_norm_act (bf16)" if out == torch.bfloat16 else "group_norm_act_bf16_f32"
    if not x_bf16 and out == torch.bfloat16:
        _chk(x)                             # the boundary into the bf16 region: an fp32 x
    else:
        _chk_bf16(x)
    _chk(gamma, beta)
    _chk_bf16(skip)
    _need(x.dim() >= 3 and x.numel() > 0 and x.shape[1] % GN_GROUPS == 0 and gamma.numel() == x.shape[1] == beta.numel()
          and (skip is None or skip.shape == x.shape),
          lambda: f"{what}: x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, skip "
                  f"{None if skip is None else tuple(skip.shape)}: {GN_GROUPS} groups over C channels, bf16 skip of x's shape")
    x, gamma, beta = _c(x), _c(gamma), _c(beta)
    skip = _c(skip) if skip is not None else None
    B, Cc = x.shape[:2]
    S = x.numel() // (B * Cc)
    stats = _gn_stats(x)
    args = (_p(x), _p(stats), _p(gamma), _p(beta), _p(skip))
    tail = (B, Cc, C.c_longlong(S), int(relu), _stream())
    if out == torch.bfloat16:
        y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
        _lib.call("ecm_gn3d_apply_bf16" if x_bf16 else "ecm_gn3d_apply_f32_bf16", *args, _p(y), *tail)
        return y
    y32 = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    y16 = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16) if out == "dual" else None
    _lib.call("ecm_gn3d_apply_bf16_f32", *args, _p(y32), _p(y16), *tail)
    return (y32, y16) if out == "dual" else y32


def _classifier_tail_bf16(x, gamma, beta, w):
    _AGG.no_grad("classifier_tail")
    _chk_bf16(x)
    _chk(gamma, beta, w)
    _need(x.dim() == 5 and x.numel() > 0 and x.shape[1] == 32 and gamma.numel() == 32 == beta.numel()
          and tuple(w.shape) == (1, 32, 3, 3, 3),
          lambda: f"classifier_tail (bf16): x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, w {tuple(w.shape)}: 32 -> 1 only")
    x, gamma, beta, w = _c(x), _c(gamma), _c(beta), _c(w)
    B, Cc, D, H, W = x.shape
    stats = _gn_stats(x)
    y = torch.empty(B, 1, D, H, W, device=x.device, dtype=torch.float32)
    _lib.call("ecm_conv3d_c1_gn_fwd_bf16", _p(x), _p(stats), _p(gamma), _p(beta), _p(w), _p(y), B, Cc, D, H, W, _stream())
    return y


# ---- opt-in bf16 inference of the 2-D feature encoder ------------------------------------------------------------------------
# Inside `with encoder_dtype(torch.bfloat16):` models.feature_extraction runs every layer after the stem convolution on bf16
# maps (csrc/bf16_encoder.hip: bf16 operands on the matrix cores, fp32 accumulation, one rounding per output); its three
# results stay fp32.  Independent of aggregation_dtype; process-wide, inference only, and the fp32 path outside the block is
# untouched.  Weights stay fp32 parameters, packed to bf16 images per call (cached under frozen_weights(), key "bf16_conv2d").
_ENC = _Bf16Switch("encoder_dtype", "the bf16 encoder")


def encoder_dtype(dtype):
    """torch.float32 (the default; a no-op) or torch.bfloat16 for the 2-D feature encoder inside the block; nests and
    restores the previous setting on exit.  bf16 is inference only: run the model under torch.no_grad()."""
    return _ENC.scope(dtype)


def encoder_bf16():
    """True inside an encoder_dtype(torch.bfloat16) block."""
    return _ENC.on()


def conv2d_bf16_supported(Ci, Co, k, stride, dil):
    """Is this Conv2d(bias=False, padding dil*(k-1)/2) inside the bf16 encoder kernel (csrc/bf16_encoder.hip)?"""
    if Ci % 16 or Co % 32 or Ci <= 0 or Co <= 0:
        return False
    if k == 3:
        return (stride == 1 and dil in (1, 2, 4)) or (stride == 2 and dil == 1)
    return k == 1 and stride in (1, 2) and dil == 1


def _pack_bf16_2d(w):
    """bf16 weight image [Ci/16][k*k][Co][16] of a Conv2d weight [Co,Ci,k,k]."""
    Co, Ci, k = w.shape[0], w.shape[1], w.shape[2]

    def build():
        wc = _c(w.detach())
        packed = torch.empty(_lib.query("ecm_conv2d_bf16_packed_elems", Ci, Co, k), device=w.device, dtype=torch.bfloat16)
        _lib.call("ecm_conv2d_bf16_pack_weight", _p(wc), _p(packed), Ci, Co, k, _stream())
        return packed
    return _cached_pack(w, "bf16_conv2d", build)


def conv2d_bf16(x, w, stride=1, dil=1, fork=False, out_dtype=torch.bfloat16):
    """Conv2d(bias=False) of the bf16 encoder on a bf16 x [B,Ci,H,W]: 3x3 (padding = dil; stride 1 with dilation 1|2|4, or
    stride 2) or 1x1 (stride 1|2).  out_dtype torch.float32: the result leaves the encoder in fp32 (rounded nowhere).
    fork=True: returns (y, x) -- x for the skip connection (no backward here)."""
    _bf16_region(_ENC, _DEC).no_grad("conv2d_bf16")
    _chk_bf16(x)
    _chk(w)
    _need(x.dim() == 4 and w.dim() == 4 and w.shape[1] == x.shape[1] and w.shape[2] == w.shape[3] and x.numel() > 0
          and conv2d_bf16_supported(x.shape[1], w.shape[0], w.shape[2], stride, dil) and out_dtype in (torch.bfloat16, torch.float32),
          lambda: f"conv2d_bf16: x {tuple(x.shape)}, w {tuple(w.shape)}, stride {stride}, dilation {dil}, out {out_dtype}: want "
                  "[B,Ci,H,W] and [Co,Ci,k,k] with Ci % 16 == 0, Co % 32 == 0, k 3 (stride 1 and dilation 1|2|4, or stride 2) "
                  "or 1 (stride 1|2)")
    x = _c(x)
    B, Ci, H, W = x.shape
    Co, k = w.shape[0], w.shape[2]
    y = torch.empty(B, Co, (H - 1) // stride + 1, (W - 1) // stride + 1, device=x.device, dtype=out_dtype)
    _lib.call("ecm_conv2d_bf16_fwd", _p(x), _p(_pack_bf16_2d(w)), _p(y), B, Ci, Co, H, W, k, int(stride), int(dil),
              int(out_dtype == torch.float32), _stream())
    return (y, x) if fork else y


def group_norm_act_bf16_f32(x, gamma, beta, skip=None, relu=False, dual=False):
    """relu?(GroupNorm32(x)*gamma+beta (+ skip)) of a bf16 x written in fp32 -- the encoder's results.  dual=True: returns
    (y32, y16), the same values also rounded to bf16 in the same pass for the next bf16 layer."""
    _ENC.no_grad("group_norm_act_bf16_f32")
    return _gn_apply_two_stage(x, gamma, beta, skip, relu, "dual" if dual else torch.float32)


# ---- opt-in bf16 inference of the cmf refinement decoder ---------------------------------------------------------------------
# Inside `with decoder_dtype(torch.bfloat16):` models.super_resolution_refinement runs on bf16 maps from conv1's GroupNorm to
# conv_out's input: its 3x3 convolutions on conv2d_bf16, its GroupNorms on the two-stage bf16 kernels, the two transposed
# convolutions and conv_out on csrc/bf16_decoder.hip; the disparities it returns are fp32, written by conv_out's kernel.
# Independent of aggregation_dtype and encoder_dtype and combinable with both (inference_dtype enters all three); a no-op for
# the architectures without a decoder.  Process-wide, inference only, and the fp32 path outside the block is untouched.
# Weights stay fp32 parameters: the transposed convolutions' bf16 images are packed per call (cached under frozen_weights(),
# key "bf16_deconv2d"), conv_out's 9*Ci weights are rounded by its kernel.
_DEC = _Bf16Switch("decoder_dtype", "the bf16 decoder")


def decoder_dtype(dtype):
    """torch.float32 (the default; a no-op) or torch.bfloat16 for cmf's refinement decoder inside the block; nests and
    restores the previous setting on exit.  bf16 is inference only: run the model under torch.no_grad()."""
    return _DEC.scope(dtype)


def decoder_bf16():
    """True inside a decoder_dtype(torch.bfloat16) block."""
    return _DEC.on()


@_contextlib.contextmanager
def inference_dtype(dtype):
    """All three bf16 inference regions at once: encoder_dtype, aggregation_dtype and decoder_dtype entered (and restored)
    together.  torch.float32 sets all three to the default."""
    with encoder_dtype(dtype), aggregation_dtype(dtype), decoder_dtype(dtype):
        yield


def deconv2d_bf16_supported(Ci, Co):
    """Is this ConvTranspose2d(Ci, Co, 3, stride 2, padding 1, output_padding 1, bias=True) inside the bf16 decoder kernel?"""
    return Ci > 0 and Ci % 16 == 0 and Co in (32, 64)


def _pack_bf16_deconv2d(w):
    """bf16 weight image [Ci/16][9][Co][16] of a ConvTranspose2d weight [Ci,Co,3,3]."""
    Ci, Co = w.shape[0], w.shape[1]

    def build():
        wc = _c(w.detach())
        packed = torch.empty(_lib.query("ecm_deconv2d_bf16_packed_elems", Ci, Co), device=w.device, dtype=torch.bfloat16)
        _lib.call("ecm_deconv2d_bf16_pack_weight", _p(wc), _p(packed), Ci, Co, _stream())
        return packed
    return _cached_pack(w, "bf16_deconv2d", build)


def deconv2d_k3s2_bias_bf16(x, w, b):
    """ConvTranspose2d(Ci, Co, 3, stride 2, padding 1, output_padding 1, bias=True) (cmf.py:236-239) of the bf16 decoder on a
    bf16 x [B,Ci,H,W] -> bf16 [B,Co,2H,2W]; w [Ci,Co,3,3] and b [Co] are the fp32 parameters (no backward here)."""
    _DEC.no_grad("deconv2d_k3s2_bias_bf16")
    _chk_bf16(x)
    _chk(w, b)
    _need(x.dim() == 4 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and w.shape[0] == x.shape[1] and x.numel() > 0
          and b.dim() == 1 and b.shape[0] == w.shape[1] and deconv2d_bf16_supported(x.shape[1], w.shape[1]),
          lambda: f"deconv2d_k3s2_bias_bf16: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}: want [B,Ci,H,W], "
                  "ConvTranspose2d's [Ci,Co,3,3] with Ci % 16 == 0, Co in {32, 64} and [Co]")
    x, b = _c(x), _c(b.detach())
    B, Ci, H, W = x.shape
    Co = w.shape[1]
    y = torch.empty(B, Co, 2 * H, 2 * W, device=x.device, dtype=torch.bfloat16)
    _lib.call("ecm_deconv2d_k3s2_bias_bf16_fwd", _p(x), _p(_pack_bf16_deconv2d(w)), _p(b), _p(y), B, Ci, Co, H, W, _stream())
    return y


def conv2d_c1_relu_bf16(x, w, b):
    """relu(Conv2d(Ci, 1, 3, 1, 1, bias=True)(x)) (cmf.py:259-264, conv_out + crap) of the bf16 decoder on a bf16 x [B,Ci,H,W]
    -> fp32 [B,1,H,W], rounded nowhere; w [1,Ci,3,3] (rounded to bf16 by the kernel) and b [1] are the fp32 parameters."""
    _DEC.no_grad("conv2d_c1_relu_bf16")
    _chk_bf16(x)
    _chk(w, b)
    _need(x.dim() == 4 and tuple(w.shape) == (1, x.shape[1], 3, 3) and b.numel() == 1 and x.numel() > 0
          and x.shape[1] % 16 == 0 and x.shape[1] <= 1024,
          lambda: f"conv2d_c1_relu_bf16: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}: want [B,Ci,H,W], "
                  "[1,Ci,3,3] and [1] with Ci % 16 == 0, Ci <= 1024")
    x, w, b = _c(x), _c(w.detach()), _c(b.detach())
    B, Ci, H, W = x.shape
    y = torch.empty(B, 1, H, W, device=x.device, dtype=torch.float32)
    _lib.call("ecm_conv2d_c1_bf16_fwd", _p(x), _p(w), _p(b), _p(y), B, Ci, H, W, _stream())
    return y
