"""The kernels that open a training step -- the shift-and-concat volume (csrc/costvol.hip) and the collapsed first convolution
(csrc/costvol_conv.hip: class weights, assembly, their adjoints) -- against fp64 on every path their host code can take.

Reached through ecm_amd.ops as the models reach them: cost_volume, ClassWeights.apply, CostvolConvAssemble.apply, costvol_conv3d and
the autograd of each.  One family of branches cannot be reached that way: ops._c copies an operand whose address is not a multiple
of 16 bytes, so the misaligned branches of the assembly (`_off` cases: every operand 4 bytes past a 16-byte boundary) are entered
through the C ABI, with the same operands and the same checks.

Reference and yardstick (tests/test_hip_numerics.py's rule, as in the other fp64 suites).
  * Exact outputs.  cost_volume forward is a copy and the assembly forward is one fp32 add per element: both must be torch.equal to
    O.cost_volume / assemble_t in fp32.
  * Summed outputs (cost_volume backward, both assembly adjoints, class weights forward and backward, costvol_conv3d and its three
    gradients).  Reference: the oracle or the closed form of tests/test_costvol_geometry.py in fp64 on the CPU.  e32(q) = the larger
    error against it of two independent fp32 evaluations, one on the CPU and the closed form on the device.  A kernel passes when
    max|q_hip - q64| <= K * e32(q) + FLOOR * max|q64|, K = 4, FLOOR = 2e-7.  Each check prints `CVRATIO <path> <quantity> <ratio>`;
    DESIGN.md section 4 holds the worst ratio per path and quantity as measured on the MI355X.
There is no exclusion of any kind: every operation here is linear.

Structure, per case: two runs on fresh operands are bit-identical; the gradient of the reference-half classes 9 and 12 (which no
(d, x) has) is exactly zero; y is exactly zero where d - x >= 3; the row-staged and the element-wise kernels give bit-identical
results on one case (aligned against `_off`).  Before each run the allocator's free blocks are filled with NaN (`poison`)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import oracle.ecm_oracle as O
import test_costvol_geometry as G
from oracle.weights import seeded
from test_costvol_geometry import ACase, CCase, KCase, XCase
from test_hip_conv3d_fp64 import DEV, FLOOR, K, cdiv  # noqa: F401  (cdiv: the suites share one)

pytestmark = pytest.mark.gpu

CASES = {**G.CONCAT, **G.ASSEMBLY, **G.WEIGHTS, **G.WHOLE}
WHOLE_WEIGHT = (32, 64, 3, 3, 3)


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def poison():
    """Fill what the caching allocator will hand out next with NaN (the idea of tests/test_hip_context_fp64.py)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 24,), float("nan"), device=DEV)] + [torch.full((1 << 14,), float("nan"), device=DEV) for _ in range(32)]
    del junk


def off4(t):
    """The same values on the device, base address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def operands(name):
    c = CASES[name]
    if isinstance(c, CCase):
        return {"L": seeded(name + ".L", c.B, c.C, c.h, c.w), "R": seeded(name + ".R", c.B, c.C, c.h, c.w),
                "G": seeded(name + ".G", c.B, 2 * c.C, c.D, c.h, c.w)}
    if isinstance(c, ACase):
        base = name[:-4] if c.off else name                                # an `_off` case has the operands of its aligned twin
        return {"P": seeded(base + ".P", c.B, G.NCP * c.Co, c.h, c.w), "Qp": seeded(base + ".Q", c.B, G.NCQ * c.Co, c.h, c.w + 2),
                "G": seeded(base + ".G", c.B, c.Co, c.D, c.h, c.w)}
    if isinstance(c, KCase):
        return {"W": seeded(name + ".W", c.Co, 2 * c.C, 3, 3, 3), "GP": seeded(name + ".GP", G.NCP * c.Co, c.C, 3, 3),
                "GQ": seeded(name + ".GQ", G.NCQ * c.Co, c.C, 3, 5)}
    return {"L": seeded(name + ".L", c.B, 32, c.h, c.w), "R": seeded(name + ".R", c.B, 32, c.h, c.w),
            "W": seeded(name + ".W", *WHOLE_WEIGHT) * (2.0 / (27 * 64)) ** 0.5, "G": seeded(name + ".G", c.B, 32, c.D, c.h, c.w)}


INPUTS = {CCase: ("L", "R"), ACase: ("P", "Qp"), KCase: ("W",), XCase: ("L", "R", "W")}
GRADS = {CCase: ("gL", "gR"), ACase: ("gP", "gQp"), KCase: ("gW",), XCase: ("gL", "gR", "gW")}
EXACT = {CCase: ("out",), ACase: ("out",), KCase: (), XCase: ()}


def path_of(c):
    if isinstance(c, CCase):
        return "concat." + G.concat_path(c.B, c.C, c.w)
    if isinstance(c, ACase):
        return "assemble.%s+%s" % (G.assemble_fwd_path(c.w, not c.off), G.assemble_bwd_path(c.D, c.w, not c.off))
    return "class_weights" if isinstance(c, KCase) else "costvol_conv3d"


def evaluate(c, o, dtype, device, closed):
    """{quantity: tensor}: the oracle where there is one (closed=False), else / otherwise the closed forms."""
    ins = [o[k].to(device=device, dtype=dtype, copy=True).requires_grad_() for k in INPUTS[type(c)]]
    if isinstance(c, CCase):
        y = G.cost_volume_t(*ins, c.D) if closed else O.cost_volume(*ins, c.D)
    elif isinstance(c, ACase):
        y = G.assemble_t(*ins, c.D)
    elif isinstance(c, KCase):
        wP, wQ = G.class_weights_t(ins[0])
        torch.autograd.backward([wP, wQ], [o["GP"].to(device=device, dtype=dtype), o["GQ"].to(device=device, dtype=dtype)])
        return {"wP": wP.detach(), "wQ": wQ.detach(), "gW": ins[0].grad}
    else:
        y = G.collapsed_t(*ins, c.D) if closed else F.conv3d(O.cost_volume(ins[0], ins[1], c.D), ins[2], None, 1, 1)
    y.backward(o["G"].to(device=device, dtype=dtype))
    return {"out": y.detach(), **{g: t.grad for g, t in zip(GRADS[type(c)], ins)}}


def assemble_abi(ecm, P, Qp, Gy, c):
    """The assembly and its adjoint through the C ABI on operands 4 bytes past a 16-byte boundary (ops._c would realign them)."""
    lib, st = ecm._lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    y = torch.empty(c.B, c.Co, c.D, c.h, c.w, device=DEV)
    gP = torch.empty(c.B, G.NCP * c.Co, c.h, c.w, device=DEV)
    gQ = torch.empty(c.B, G.NCQ * c.Co, c.h, c.w + 2, device=DEV)
    Po, Qo, Go = off4(P), off4(Qp), off4(Gy)
    lib.call("ecm_costvol_conv_assemble_fwd", p(Po), p(Qo), p(y), c.B, c.Co, c.D, c.h, c.w, st)
    lib.call("ecm_costvol_conv_assemble_bwd", p(Go), p(gP), p(gQ), c.B, c.Co, c.D, c.h, c.w, st)
    torch.cuda.synchronize()
    return {"out": y, "gP": gP, "gQp": gQ}


def hip(ecm, c, o):
    ops = ecm.ops
    poison()
    if isinstance(c, ACase) and c.off:
        return assemble_abi(ecm, o["P"], o["Qp"], o["G"], c)
    ins = [o[k].to(DEV).requires_grad_() for k in INPUTS[type(c)]]
    assert all(t.data_ptr() % 16 == 0 for t in ins)
    if isinstance(c, KCase):
        wP, wQ = ops.ClassWeights.apply(ins[0])
        torch.autograd.backward([wP, wQ], [o["GP"].to(DEV), o["GQ"].to(DEV)])
        out = {"wP": wP.detach(), "wQ": wQ.detach(), "gW": ins[0].grad}
    else:
        if isinstance(c, CCase):
            y = ops.cost_volume(*ins, c.D)
        elif isinstance(c, ACase):
            y = ops.CostvolConvAssemble.apply(*ins, c.D)
        else:
            y = ops.costvol_conv3d(*ins, c.D)
        y.backward(o["G"].to(DEV))
        out = {"out": y.detach(), **{g: t.grad for g, t in zip(GRADS[type(c)], ins)}}
    for k, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous(), k
    return out


def structure_checks(name, c, a, fails):
    if isinstance(c, (ACase, XCase)):
        D, w = c.D, c.w
        _, _, _, valid = G.class_index(D, w)
        dead = ~valid                                                          # [D, w]: d - x >= 3
        y = a["out"].cpu()
        if dead.any() and not bool((y.permute(0, 1, 3, 2, 4)[..., dead] == 0).all()):
            fails.append(f"{name}: y is not exactly zero where d - x >= 3")
    if isinstance(c, ACase):
        gP = a["gP"].cpu().view(c.B, G.NCP, c.Co, c.h, c.w)
        if not bool((gP[:, list(G.UNREACHABLE_P)] == 0).all()):
            fails.append(f"{name}: gP of the classes {G.UNREACHABLE_P} is not exactly zero")
        touched = G.classes_touched(c.w, c.D)[0]
        for k in range(G.NCP):
            if k not in touched and not bool((gP[:, k] == 0).all()):
                fails.append(f"{name}: gP of class {k}, which no (d, x) of this shape has, is not exactly zero")


def run_case(ecm, name):
    c = CASES[name]
    o = operands(name)
    fails, runs = [], None
    try:
        runs = [hip(ecm, c, o) for _ in range(2)]
        a, b = runs
        q64 = evaluate(c, o, torch.float64, "cpu", False)
        draws = [evaluate(c, o, torch.float32, "cpu", False), evaluate(c, o, torch.float32, DEV, True)]
        assert set(a) == set(q64)
        for k, got in a.items():
            ref = q64[k]
            assert got.shape == ref.shape, k
            if not torch.equal(got, b[k]):
                fails.append(f"{name}: {k} differs between two runs in {int((got != b[k]).sum())} elements")
            if k in EXACT[type(c)]:
                want = draws[0][k]
                same = torch.equal(got.cpu(), want)
                print(f"CVEXACT {path_of(c)} {k} {'equal' if same else 'DIFFERENT'}   # {name}")
                if not same:
                    bad = got.cpu() != want
                    fails.append(f"{name}: {k} on {path_of(c)} is not bit-identical to the fp32 reference in {int(bad.sum())} elements, "
                                 f"first at {tuple(int(v) for v in bad.nonzero()[0])}")
                continue
            each = [float((d[k].cpu().double() - ref).abs().max()) for d in draws]
            e32, scale = max(each), float(ref.abs().max())
            err = float((got.cpu().double() - ref).abs().max())
            bound = K * e32 + FLOOR * scale
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            print(f"CVRATIO {path_of(c)} {k} {ratio:.3f}   # {name}: err {err:.3e}, e32 {e32:.3e} [{each[0]:.2e} {each[1]:.2e}], max|ref| {scale:.3e}")
            if not err <= bound:                                     # (a NaN fails)
                fails.append(f"{name}: {k} on {path_of(c)}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")
        structure_checks(name, c, a, fails)
        if isinstance(c, ACase) and c.off:                       # the same operands, aligned, through ops: the other kernels
            twin = hip(ecm, c._replace(off=False), o)
            assert path_of(c._replace(off=False)) != path_of(c) or G.fwd_lds_bytes(c.w) > G.LDS_MAX
            for k, t in a.items():
                if not torch.equal(t, twin[k]):
                    fails.append(f"{name}: {k} is not bit-identical between the aligned and the 4-byte-offset operands")
        ecm.ops.check_async_errors()
        assert not fails, "\n".join(fails)
    finally:
        del runs


def test_case_table_covers_every_class():
    assert G.missing_classes() == []


def test_ops_realign_a_misaligned_operand(ecm):
    """Why the `_off` cases go through the C ABI: ops hands the kernels 16-byte-aligned operands only."""
    t = off4(seeded("cv.align", 2, 15, 1, 4))
    assert ecm.ops._c(t).data_ptr() % 16 == 0 and torch.equal(ecm.ops._c(t), t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_costvol_fp64(ecm, name):
    """Every output and gradient of one case of the table: exact or under the fp64 bound, exact structure, bit-identical repeats."""
    run_case(ecm, name)
