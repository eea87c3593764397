"""The split-bf16 kernels of csrc/split_bf16.hip (ops.split_products) against fp64, on every path of the case table that
tests/test_split_bf16_cpu.py asserts complete.

Yardstick: the one of tests/test_hip_conv3d_fp64.py, restated.  Reference: F.conv3d / F.conv_transpose3d and autograd in fp64 on
the CPU; operands from oracle.weights.seeded, weights He-scaled.  Unit: the reference's OWN fp32 error, e32(q) = max |q32 - q64|
over independent fp32 evaluations of the same expression -- torch's on the CPU, torch's on the device and, for what a stride-2
convolution computes (the convolution's y, the transposed convolution's gx), `chain_conv`: the fp32 kernel's summation order (one
mul-then-add chain over chunks of 2 channels x 27 taps) in plain torch.  e32 never comes from the code under test.  A quantity
passes when  max|q_hip - q64| <= 4 * e32(q) + 2e-7 * max|q64|  -- the bound the fp32 kernels meet, which is what
"fp32-equivalent" means here.  Each comparison prints `SPRATIO <case> <quantity> <ratio>`; DESIGN.md section 14 holds the worst
(measured on the MI355X: 0.73 for the transposed kernel's y, 0.65 for its gx role, 0.31 / 0.25 for the stride-2 kernel's)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from oracle.weights import seeded
from test_split_bf16_cpu import CONV_CASES, DECONV_CASES

pytestmark = pytest.mark.gpu

K, FLOOR = 4.0, 2e-7
DEV = "cuda"
ALL = ("conv_fwd", "conv_dgrad", "deconv_fwd", "deconv_dgrad")
SPLIT_SYMS = {"ecm_conv3d_k3s2_split_fwd", "ecm_deconv3d_k3s2_split_fwd", "ecm_conv3d_split_pack_weight"}
FP32_SYMS = {"ecm_conv3d_k3_fwd", "ecm_deconv3d_k3s2_fwd"}
ECM_EUNSUP = -2


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


@contextlib.contextmanager
def recorder(ecm):
    """Names of every entry launched through _lib.call inside the block."""
    names, real = [], ecm._lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    ecm._lib.call = call
    try:
        yield names
    finally:
        ecm._lib.call = real


def out_dims(dims, stride=2):
    return tuple((d - 1) // stride + 1 for d in dims)


def chain_conv(x, w, stride, cic):
    """conv3d(x, w, stride, pad 1) as the fp32 kernel sums it: one chain per output over (chunk of cic channels, tap, channel)."""
    B, Ci = x.shape[:2]
    o = out_dims(x.shape[2:], stride)
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    acc = x.new_zeros(B, w.shape[0], *o)
    for c0 in range(0, Ci, cic):
        for kd, kh, kw in ((a, b, c) for a in range(3) for b in range(3) for c in range(3)):
            for c in range(c0, min(c0 + cic, Ci)):
                win = xp[:, c:c + 1, kd:kd + (o[0] - 1) * stride + 1:stride, kh:kh + (o[1] - 1) * stride + 1:stride,
                         kw:kw + (o[2] - 1) * stride + 1:stride]
                acc = acc + w[:, c, kd, kh, kw].view(1, -1, 1, 1, 1) * win
    return acc


def _operands(name, op, B, Ci, Co, dims, odims, fork):
    x = seeded("sp." + name + ".x", B, Ci, *dims)
    wshape = (Ci, Co) if op == "deconv" else (Co, Ci)
    w = seeded("sp." + name + ".w", *wshape, 3, 3, 3) * (2.0 / (27 * Ci)) ** 0.5
    G = seeded("sp." + name + ".G", B, Co, *odims)
    Gs = seeded("sp." + name + ".Gs", *x.shape) if fork else None
    return x, w, G, Gs


def _torch(op, odims, x, w, G, Gs, dtype, device):
    cv = lambda t: t.detach().to(device=device, dtype=dtype, copy=True)                 # noqa: E731
    xs, ws = cv(x).requires_grad_(), cv(w).requires_grad_()
    if op == "deconv":
        opad = tuple(o - (2 * n - 1) for o, n in zip(odims, x.shape[2:]))
        y = F.conv_transpose3d(xs, ws, None, 2, 1, opad)
    else:
        y = F.conv3d(xs, ws, None, 2, 1)
    y.backward(cv(G))
    return {"y": y.detach(), "gx": xs.grad if Gs is None else xs.grad + cv(Gs), "gw": ws.grad}


def _hip(ecm, op, x, w, G, Gs, mode, kinds=ALL):
    """The operation through ecm_amd.ops on fresh copies of the operands; returns the results and the entries launched."""
    ops = ecm.ops
    xg, wg, Gd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), G.to(DEV)
    with recorder(ecm) as names, ops.split_products(mode, kinds):
        if op == "deconv":
            y = ops.deconv3d_k3s2(xg, wg)
        elif Gs is not None:
            y, xa = ops.conv3d_k3(xg, wg, 2, fork=True)
        else:
            y = ops.conv3d_k3(xg, wg, 2)
        if Gs is not None:
            torch.autograd.backward([y, xa], [Gd, Gs.to(DEV)])
        else:
            y.backward(Gd)
        ops.join_side_streams()
    assert y.dtype == xg.grad.dtype == wg.grad.dtype == torch.float32 and y.shape == Gd.shape
    return {"y": y.detach(), "gx": xg.grad, "gw": wg.grad}, set(names)


def _compare(label, hip, q64, e32, fails):
    for k, got in hip.items():
        ref = q64[k]
        err = float((got.cpu().double() - ref).abs().max())
        scale = float(ref.abs().max())
        bound = K * e32[k] + FLOOR * scale
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"SPRATIO {label} {k} {ratio:.3f}   # err {err:.3e}, e32 {e32[k]:.3e}, max|ref| {scale:.3e}")
        if not err <= bound:
            fails.append(f"{label}: {k}: |hip - fp64| = {err:.3e} > {K} * {e32[k]:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")


def _e32(op, odims, x, w, G, Gs, q64, chain_keys):
    draws = [_torch(op, odims, x, w, G, Gs, torch.float32, "cpu"), _torch(op, odims, x, w, G, Gs, torch.float32, DEV)]
    chain = {}
    if "y" in chain_keys:
        chain["y"] = chain_conv(x.to(DEV), w.to(DEV), 2, 2)
    if "gx" in chain_keys:      # Deconv3dK3S2.backward: the stride-2 convolution of G by the same weight read as [Cout, Cin]
        chain["gx"] = chain_conv(G.to(DEV), w.to(DEV), 2, 2)
    e = {}
    for k in q64:
        cand = [d[k] for d in draws] + ([chain[k]] if k in chain else [])
        e[k] = max(float((c.cpu().double() - q64[k]).abs().max()) for c in cand)
    return e


# ---- 1. through ops inside the switch -------------------------------------------------------------------------------------------
OPS_CASES = {**{n: ("conv",) + c for n, c in CONV_CASES.items() if c[-1] == "ops"},
             **{n: ("deconv",) + c for n, c in DECONV_CASES.items() if c[-1] == "ops"}}


# fork=True exists on ops.conv3d_k3 only
OPS_RUNS = [(n, f) for n in sorted(OPS_CASES) for f in ((False, True) if OPS_CASES[n][0] == "conv" else (False,))]


@pytest.mark.parametrize("name,fork", OPS_RUNS, ids=[n + ("+fork" if f else "") for n, f in OPS_RUNS])
def test_ops_inside_the_switch(ecm, name, fork):
    op, B, Ci, Co, dims, odims, _ = OPS_CASES[name]
    x, w, G, Gs = _operands(name, op, B, Ci, Co, dims, odims, fork)
    (a, na), (b, _) = [_hip(ecm, op, x, w, G, Gs, "bf16x3") for _ in range(2)]
    off, noff = _hip(ecm, op, x, w, G, Gs, "fp32")
    q64 = _torch(op, odims, x, w, G, Gs, torch.float64, "cpu")
    e32 = _e32(op, odims, x, w, G, Gs, q64, {"y"} if op == "conv" else {"gx"})
    fails = []
    _compare(f"{name}{'+fork' if fork else ''}", a, q64, e32, fails)
    for k in a:
        if not torch.equal(a[k], b[k]):
            fails.append(f"{name}: {k} differs between two runs in {int((a[k] != b[k]).sum())} elements")
    if not torch.equal(a["gw"], off["gw"]):
        fails.append(f"{name}: gw moved with the switch (the weight gradients stay on the fp32 kernels)")
    want = {"ecm_conv3d_k3s2_split_fwd", "ecm_deconv3d_k3s2_split_fwd", "ecm_conv3d_split_pack_weight"}
    if not want <= na:
        fails.append(f"{name}: inside the block launched {sorted(na)}")
    if na & FP32_SYMS or noff & SPLIT_SYMS or not FP32_SYMS <= noff:
        fails.append(f"{name}: wrong entries: inside {sorted(na)}, outside {sorted(noff)}")
    if a["y"].numel() * Ci >= 4096:      # random cases with enough outputs that an identical fp32 result is not chance
        for k in ("y", "gx"):
            if torch.equal(a[k], off[k]):
                fails.append(f"{name}: {k} inside the block is bit-identical to the fp32 kernel's: a silent fallback?")
    ecm.ops.check_async_errors()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ALL)
def test_each_kind_alone(ecm, kind):
    """kinds= selects exactly the named kernel; the other three quantities stay bit-identical to the fp32 path."""
    op = "conv" if kind.startswith("conv") else "deconv"
    name = "c_odd" if op == "conv" else "t_ragged"
    _, B, Ci, Co, dims, odims, _ = OPS_CASES[name]
    x, w, G, _ = _operands(name, op, B, Ci, Co, dims, odims, False)
    on, names = _hip(ecm, op, x, w, G, None, "bf16x3", (kind,))
    off, _ = _hip(ecm, op, x, w, G, None, "fp32")
    moved = "y" if kind.endswith("fwd") else "gx"
    sym = "ecm_conv3d_k3s2_split_fwd" if kind in ("conv_fwd", "deconv_dgrad") else "ecm_deconv3d_k3s2_split_fwd"
    assert sym in names and len(names & SPLIT_SYMS) == 2, sorted(names)
    for k in ("y", "gx", "gw"):
        assert torch.equal(on[k], off[k]) == (k != moved), k


# ---- the C-ABI cases: 2n-1 outputs of the transposed kernel and the adjoint pack mode ---------------------------------------------
ABI_CASES = {**{n: ("conv",) + c for n, c in CONV_CASES.items() if c[-1] == "abi"},
             **{n: ("deconv",) + c for n, c in DECONV_CASES.items() if c[-1] == "abi"}}


def _abi_run(ecm, op, x, w, Co, odims, guard=256):
    """One launch below ops' autograd into a NaN-poisoned buffer with guard bands; returns y and the untouched-guards verdict."""
    ops = ecm.ops
    xd, wd = x.to(DEV).contiguous(), w.to(DEV).contiguous()
    n = x.shape[0] * Co * odims[0] * odims[1] * odims[2]
    buf = torch.full((guard + n + guard,), float("nan"), device=DEV)
    y = buf[guard:guard + n].view(x.shape[0], Co, *odims)
    packed = ops._pack_split(wd, op == "deconv")
    B, Ci, D, H, W = x.shape
    if op == "deconv":
        ecm._lib.call("ecm_deconv3d_k3s2_split_fwd", ops._p(xd), ops._p(packed), ops._p(y), B, Ci, Co, D, H, W, *odims, ops._stream())
    else:
        ecm._lib.call("ecm_conv3d_k3s2_split_fwd", ops._p(xd), ops._p(packed), ops._p(y), B, Ci, Co, D, H, W, ops._stream())
    torch.cuda.synchronize()
    clean = bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
    return y.clone(), clean


@pytest.mark.parametrize("name", sorted(ABI_CASES))
def test_c_abi_cases(ecm, name):
    """The transposed kernel's 2n-1 outputs, and a ConvTranspose3d weight [Ci,Co,27] read as a Conv3d operand [Cout,Cin,27] (the
    adjoint pack mode of Deconv3dK3S2.backward), at extents ops' autograd cannot produce."""
    op, B, Ci, Co, dims, odims, _ = ABI_CASES[name]
    x, w, G, _ = _operands(name, op, B, Ci, Co, dims, odims, False)
    # (op == "conv": w [Co,Ci,27] holds the bytes of a ConvTranspose3d weight [Ci_t = Co, Co_t = Ci]; pack mode 0 reads it as Conv3d's)
    runs = [_abi_run(ecm, op, x, w, Co, odims) for _ in range(2)]
    q64 = {"y": _torch(op, odims, x, w, G, None, torch.float64, "cpu")["y"]}
    e32 = _e32(op, odims, x, w, G, None, q64, {"y"} if op == "conv" else set())
    fails = []
    _compare(name, {"y": runs[0][0]}, q64, e32, fails)
    assert runs[0][1] and runs[1][1], "wrote outside y"
    assert not torch.isnan(runs[0][0]).any(), "left part of y unwritten"
    assert torch.equal(runs[0][0], runs[1][0])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", sorted(OPS_CASES))
def test_guard_bands(ecm, name):
    """Outputs allocated NaN-poisoned between guard bands: every element of y is written, nothing outside it is, and the result
    is the one ops returns, bit for bit."""
    op, B, Ci, Co, dims, odims, _ = OPS_CASES[name]
    x, w, G, _ = _operands(name, op, B, Ci, Co, dims, odims, False)
    y, clean = _abi_run(ecm, op, x, w, Co, odims)
    assert clean, "wrote outside y"
    assert not torch.isnan(y).any(), "left part of y unwritten"
    with ecm.ops.split_products("bf16x3", ALL), torch.no_grad():
        ref = ecm.ops.deconv3d_k3s2(x.to(DEV), w.to(DEV)) if op == "deconv" else ecm.ops.conv3d_k3(x.to(DEV), w.to(DEV), 2)
    assert torch.equal(y, ref)


# ---- 2. special values ----------------------------------------------------------------------------------------------------------
def _one_hot(ecm, op, xv, wv):
    """One non-zero input voxel and one non-zero weight; returns (y, fp64 reference)."""
    Ci, Co, dims = 32, 64, (3, 3, 3)
    x = torch.zeros(1, Ci, *dims)
    x[0, 5, 1, 1, 1] = xv
    w = torch.zeros(*((Ci, Co) if op == "deconv" else (Co, Ci)), 3, 3, 3)
    w[(5, 37) if op == "deconv" else (37, 5)][2, 0, 2] = wv
    with ecm.ops.split_products("bf16x3", ALL), torch.no_grad():
        y = ecm.ops.deconv3d_k3s2(x.to(DEV), w.to(DEV)) if op == "deconv" else ecm.ops.conv3d_k3(x.to(DEV), w.to(DEV), 2)
    ref = F.conv_transpose3d(x.double(), w.double(), None, 2, 1, 1) if op == "deconv" else F.conv3d(x.double(), w.double(), None, 2, 1)
    return y.cpu().double(), ref


MANT_X, MANT_W = 1.0 + (2 ** 23 - 3) / 2 ** 23, -(1.0 + 5592405 / 2 ** 23)      # full-mantissa significands (…1101, 0101…)


@pytest.mark.parametrize("op", ["conv", "deconv"])
def test_single_product_is_fp32_accurate(ecm, op):
    """2a.  Every output equals x*w within 2^-21 relative: the dropped x2w3 and x3w2 are <= 2^-24 each, x3w3 2^-32, and six fp32
    accumulations <= 2^-24 each -- under 2^-21 in all.  Measured worst: 3.6e-8 on both kernels."""
    worst, fails = 0.0, []
    for ex in (-60, 0, 60):
        for ew in (-60, 0, 60):
            for sx in (1.0, -1.0):
                xv, wv = float(torch.tensor(sx * MANT_X * 2.0 ** ex)), float(torch.tensor(MANT_W * 2.0 ** ew))
                y, ref = _one_hot(ecm, op, xv, wv)
                assert int((ref != 0).sum()) == 1
                rel = float(((y - ref).abs() / abs(xv * wv)).max())
                worst = max(worst, rel)
                print(f"SPONE {op} x=2^{ex} w=2^{ew} sign {sx:+.0f}: rel err {rel:.3e} (2^-21 = {2.0 ** -21:.3e})")
                if not rel <= 2.0 ** -21:
                    fails.append(f"{op} x=2^{ex} w=2^{ew}: rel err {rel:.3e}")
    print(f"SPONE {op} worst {worst:.3e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("op", ["conv", "deconv"])
def test_tiny_operand_is_reported(ecm, op):
    """2b.  |x| = 2^-115: below the guaranteed range (2^-110), x's third term is a bf16 subnormal.  Reported, not gated: the figure
    says whether the matrix core flushes bf16-subnormal operands.  Measured: 1.75e-6 on both kernels = the
    bits of x under 2^-133 alone; a flushed third term would cost 1.5e-5, so it is not flushed."""
    for ew in (0, 60):
        xv, wv = float(torch.tensor(MANT_X * 2.0 ** -115)), float(torch.tensor(MANT_W * 2.0 ** ew))
        y, ref = _one_hot(ecm, op, xv, wv)
        rel = float(((y - ref).abs() / abs(xv * wv)).max())
        print(f"SPTINY {op} x=2^-115 w=2^{ew}: rel err {rel:.3e} (2^-21 = {2.0 ** -21:.3e}, 2^-16 = {2.0 ** -16:.3e}, 2^-8 = {2.0 ** -8:.3e})")
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("op", ["conv", "deconv"])
def test_non_finite_inputs_stay_local(ecm, op):
    """2c.  One +Inf and one NaN input voxel: exactly the outputs whose receptive field holds one are non-finite, every other
    output equals the run without them bit for bit (no Inf - Inf from the split, no 0 * Inf from the pad slot)."""
    name = "c_odd" if op == "conv" else "t_ragged"
    _, B, Ci, Co, dims, odims, _ = OPS_CASES[name]
    x, w, _, _ = _operands(name, op, B, Ci, Co, dims, odims, False)
    xs = x.clone()
    xs[0, 3, 0, 0, 0] = float("inf")
    xs[0, Ci - 1, dims[0] - 1, dims[1] - 1, dims[2] - 2] = float("nan")
    run = lambda t: (ecm.ops.deconv3d_k3s2(t.to(DEV), w.to(DEV)) if op == "deconv" else ecm.ops.conv3d_k3(t.to(DEV), w.to(DEV), 2)).cpu()   # noqa: E731
    with ecm.ops.split_products("bf16x3", ALL), torch.no_grad():
        plain, special = run(x), run(xs)
    ind = (~torch.isfinite(xs)).double().sum(1, keepdim=True)
    ones = torch.ones(1, 1, 3, 3, 3, dtype=torch.float64)
    touched = (F.conv_transpose3d(ind, ones, None, 2, 1, 1) if op == "deconv" else F.conv3d(ind, ones, None, 2, 1)) > 0
    touched = touched.expand_as(plain)
    assert torch.isfinite(plain).all() and 0 < int(touched.sum()) < touched.numel()
    assert torch.equal(~torch.isfinite(special), touched)
    assert torch.equal(special[~touched], plain[~touched])


# ---- 3. robustness --------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes(ecm):
    """Ci = 16 / Co = 48: ECM_EUNSUP from the C entries; through ops inside the block, the fp32 kernels."""
    ops, lib = ecm.ops, ecm._lib.load()
    x = seeded("sp.un.x", 1, 16, 3, 5, 9).to(DEV)
    w = (seeded("sp.un.w", 48, 16, 3, 3, 3) * 0.05).to(DEV)
    wt = (seeded("sp.un.wt", 16, 48, 3, 3, 3) * 0.05).to(DEV)
    y = torch.empty(1, 48, 6, 10, 18, device=DEV)
    pk = torch.empty(1 << 16, device=DEV, dtype=torch.bfloat16)
    assert lib.ecm_conv3d_k3s2_split_fwd(ops._p(x), ops._p(pk), ops._p(y), 1, 16, 48, 3, 5, 9, None) == ECM_EUNSUP
    assert lib.ecm_deconv3d_k3s2_split_fwd(ops._p(x), ops._p(pk), ops._p(y), 1, 16, 48, 3, 5, 9, 6, 10, 18, None) == ECM_EUNSUP
    assert lib.ecm_deconv3d_k3s2_split_fwd(ops._p(x), ops._p(pk), ops._p(y), 1, 64, 64, 3, 5, 9, 7, 10, 18, None) == ECM_EUNSUP
    with recorder(ecm) as names, ops.split_products("bf16x3", ALL), torch.no_grad():
        a, b = ops.conv3d_k3(x, w, 2), ops.deconv3d_k3s2(x, wt)
        c = ops.conv3d_k3(seeded("sp.un.x1", 1, 32, 3, 5, 9).to(DEV), (seeded("sp.un.w1", 32, 32, 3, 3, 3) * 0.05).to(DEV), 1)
    assert not set(names) & SPLIT_SYMS, names
    with torch.no_grad():
        assert torch.equal(a, ops.conv3d_k3(x, w, 2)) and torch.equal(b, ops.deconv3d_k3s2(x, wt)) and c.shape == (1, 32, 3, 5, 9)


def test_switch_off_is_the_fp32_entries(ecm):
    """Outside the block a stride-2 convolution and a transposed convolution are the fp32 entries' results, bit for bit."""
    ops = ecm.ops
    x = seeded("sp.off.x", 1, 32, 5, 9, 35).to(DEV)
    w = (seeded("sp.off.w", 64, 32, 3, 3, 3) * 0.05).to(DEV)
    wt = (seeded("sp.off.wt", 32, 64, 3, 3, 3) * 0.05).to(DEV)
    assert not ops.split_products_on()
    with torch.no_grad():
        assert torch.equal(ops.conv3d_k3(x, w, 2), ops._conv_fwd(x, ops._pack_conv(w), 64, 2))
        assert torch.equal(ops.deconv3d_k3s2(x, wt), ops._deconv_fwd(x, ops._pack_deconv(wt), 64, (10, 18, 70)))


def test_frozen_weights_cache_covers_split_layouts(ecm):
    ops = ecm.ops
    x = seeded("sp.fz.x", 1, 32, 3, 5, 9).to(DEV)
    w = (seeded("sp.fz.w", 64, 32, 3, 3, 3) * 0.05).to(DEV)
    with ops.split_products("bf16x3", ALL), torch.no_grad(), ops.frozen_weights():
        with recorder(ecm) as n1:
            a = ops.conv3d_k3(x, w, 2)
        with recorder(ecm) as n2:
            b = ops.conv3d_k3(x, w, 2)
        ops.invalidate_packed()
        with recorder(ecm) as n3:
            c = ops.conv3d_k3(x, w, 2)
    assert "ecm_conv3d_split_pack_weight" in n1 and "ecm_conv3d_split_pack_weight" not in n2 and "ecm_conv3d_split_pack_weight" in n3
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- 4. the whole model ---------------------------------------------------------------------------------------------------------
def _cmfsm(ecm):
    from oracle.weights import tensor_for
    model = ecm.get_model("cmfsm")
    model.load_state_dict({k: tensor_for(k, v.shape) for k, v in model.state_dict().items()})
    return model.cuda().train()


def test_cmfsm_train_step_inside_the_switch(ecm):
    """cmfsm forward, stereo_loss3 and backward at 256x512 inside the block against fixture g8d: the rule
    tests/test_hip_fp64_yardstick.py applies to the fp32 path there -- disparities within max 2e-3 px / mean 1e-4 * i + 1e-4 px of
    fp64, the loss within 4 x the reference-fp32's distance + 1e-5, every parameter gradient within 4 x the reference-fp32's own
    distance + 1e-3 of scale (norm, projection, full tensors: its _check_params)."""
    from test_hip_fp64_yardstick import _check_params, _z
    z = _z("g8d_full_cmfsm_256x512_fp64")
    model = _cmfsm(ecm)
    left, right = seeded("g8.left", 1, 3, 256, 512).cuda(), seeded("g8.right", 1, 3, 256, 512).cuda()
    gt = (torch.rand(1, 256, 512, generator=torch.Generator().manual_seed(8)) * 191.0).cuda()
    with recorder(ecm) as names, ecm.ops.split_products("bf16x3", ALL):
        o = model(left, right)
        loss, _ = ecm.ops.stereo_loss3(o, gt, 192)
        loss.backward()
        ecm.ops.join_side_streams()
    ecm.ops.check_async_errors()
    # three hourglasses x (conv1, conv3, conv5, conv6), forward and data gradient
    assert names.count("ecm_conv3d_k3s2_split_fwd") >= 6 and names.count("ecm_deconv3d_k3s2_split_fwd") >= 6, \
        (names.count("ecm_conv3d_k3s2_split_fwd"), names.count("ecm_deconv3d_k3s2_split_fwd"))
    for i in (1, 2, 3):
        d64 = (o[i - 1].detach().double().cpu()[..., ::4, ::4] - torch.from_numpy(z[f"o{i}_64"])).abs()
        print(f"SPMODEL o{i}: max {float(d64.max()):.3e} mean {float(d64.mean()):.3e}")
        assert float(d64.max()) <= 2e-3 and float(d64.mean()) <= 1e-4 * i + 1e-4, (i, float(d64.max()), float(d64.mean()))
    l64, l32 = float(z["loss_64"]), float(z["loss_32"])
    assert abs(float(loss.detach()) - l64) <= K * abs(l32 - l64) + 1e-5 * l64, (float(loss.detach()), l64, l32)
    n_full, worst = _check_params(model, z, "cmfsm split")
    assert n_full >= 14, n_full
    print("SPMODEL worst norm-error ratios vs the yardstick:", worst)


def test_ddp_step_inside_the_switch(ecm):
    """One step of FlatBucketDDP + fused Adam with the weight-gradient side stream on, inside the block: finite loss and
    parameters, and the split kernels ran."""
    from importlib import import_module
    D = import_module("explicit-context-mapping-for-stereo-matching_amd.dist")
    ops = ecm.ops
    model = _cmfsm(ecm)
    prev = ops.WGRAD_OVERLAP
    ddp = D.FlatBucketDDP(model, 1)                            # turns the side stream on
    opt = torch.optim.Adam(ddp.params, lr=1e-4, fused=True)
    left, right = seeded("g8.left", 1, 3, 256, 512).cuda(), seeded("g8.right", 1, 3, 256, 512).cuda()
    gt = (torch.rand(1, 256, 512, generator=torch.Generator().manual_seed(8)) * 191.0).cuda()
    try:
        with recorder(ecm) as names, ops.split_products("bf16x3", ALL):
            ddp.zero_grad()
            loss, count = D.masked_smooth_l1_x3_with_count(model(left, right), gt, 192)
            ddp.global_mean_loss(loss, count).backward()
            ddp.allreduce_gradients()
            opt.step()
        torch.cuda.synchronize()
        ops.check_async_errors()
        assert "ecm_conv3d_k3s2_split_fwd" in names and "ecm_deconv3d_k3s2_split_fwd" in names
        assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        ops.enable_wgrad_overlap(prev)
        ops._SIDE.clear()


def test_graphed_forward_replay_equals_eager(ecm):
    """Under dist.GraphedForward the block's kernels are captured: the replay equals the eager forward bit for bit (eager on the
    two-stage GroupNorm kernels, which are what a capture records: like against like)."""
    from importlib import import_module
    D = import_module("explicit-context-mapping-for-stereo-matching_amd.dist")
    ops = ecm.ops
    model = _cmfsm(ecm).eval()
    left, right = seeded("g8.left", 1, 3, 256, 512).cuda(), seeded("g8.right", 1, 3, 256, 512).cuda()
    with ops.split_products("bf16x3", ALL):
        with recorder(ecm) as names:
            graphed = D.GraphedForward(model, left, right)
        assert "ecm_conv3d_k3s2_split_fwd" in names and "ecm_deconv3d_k3s2_split_fwd" in names
        got = [t.clone() for t in graphed(left, right)]
        old = ops.gn_cluster_mode(0)
        try:
            with torch.no_grad():
                want = model(left, right)
        finally:
            ops.gn_cluster_mode(old)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    ops.check_async_errors()


# ---- 5. the variant architectures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["cmfsm_sub_8", "cm_sub_16"])
def test_variant_hourglasses_reach_the_path(ecm, arch):
    """The post-encoder path of two variant architectures at their fixture sizes inside the block: the predictions within the
    arch tests' tolerance of the reference's (tests/test_hip_parity.py: max 2e-2 px, mean 1e-3 px), and the split kernels ran."""
    from conftest import load_golden
    from test_oracle_golden import arch_inputs, arch_sd
    g = load_golden(f"arch_{arch}")
    model = ecm.get_model(arch)
    missing, unexpected = model.load_state_dict(arch_sd(arch), strict=False)
    assert not unexpected and all(k.startswith("feature_extraction") for k in missing)
    model = model.cuda()
    feats = [t.cuda() for t in arch_inputs(arch)]
    with recorder(ecm) as names, ecm.ops.split_products("bf16x3", ALL), torch.no_grad():
        preds = model.hot_path(*feats)
    assert "ecm_conv3d_k3s2_split_fwd" in names and "ecm_deconv3d_k3s2_split_fwd" in names, sorted(set(names))
    for i, p in enumerate(preds, 1):
        d = (p.detach().cpu() - g[f"pred{i}"]).abs()
        print(f"SPARCH {arch} pred{i}: max {float(d.max()):.3e} mean {float(d.mean()):.3e}")
        assert p.shape == g[f"pred{i}"].shape and d.max() <= 2e-2 and d.mean() <= 1e-3, (arch, i, float(d.max()), float(d.mean()))
