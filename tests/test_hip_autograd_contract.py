"""The layer between autograd and the C ABI -- the torch.autograd.Function classes of ops.py -- under the callers the fp64 suites
do not have: partial gradients, odd operand and gradient layouts, unused outputs, accumulation, refused operands.

One table (tests/autograd_contract_table.py; tests/test_autograd_contract_cpu.py holds it to ops.py) has a row per Function and
backward branch; shapes are taken by name from the fp64 suites' case tables, references are those suites' own.

The canonical run of a row: contiguous, aligned operands, every differentiable input requires a gradient, every output is used,
the output gradient is a dense seeded G.  It is checked once against fp64 with the project's yardstick,
|hip - fp64| <= K * e32 + FLOOR * max|fp64| (K = 4, FLOOR = 2e-7, e32 the reference's own fp32 error over torch on the CPU, torch
on the device and, for the convolutions, the fp64 suites' restatements of the kernel's summation order).

Every variant is then held to the canonical run by torch.equal, on every output and every gradient it still produces: a variant
changes which launches happen and where the operands live, never a value, and the kernels sum in a fixed order.  No element is
excluded.  Every run goes through tests/test_hip_abi_calls.py's recorder (census=False, strict=True): a pointer to a strided or
misplaced tensor is a Python failure that names the argument, before anything is launched.

V1 gradient subsets, V2 operand layouts, V3 gradient layouts, V4 unused outputs, V5 accumulation, V6 refusals: DESIGN.md,
"The autograd contract"."""
import contextlib
import itertools

import pytest
import torch
import torch.nn.functional as F

import oracle.ecm_oracle as O
import test_costvol_geometry as CG
import test_hip_context_fp64 as CM
import test_hip_conv2d_fp64 as C2
import test_hip_conv3d_fp64 as C3
import test_hip_groupnorm_fp64 as GN
import test_hip_split_bf16_fp64 as SP
import test_split_bf16_cpu as SPC
from autograd_contract_table import ACCUMULATION_ROWS, CONTEXT_SUBSETS, OVERLAP_ROWS, ROWS
from oracle.weights import seeded
from test_hip_abi_calls import recording
from test_hip_variants_fullsize import soft_argmin_t, trilinear_t, volume_mapping_t

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, FLOOR = C3.K, C3.FLOOR
OWN_CALLS = {"ecm_async_status", "ecm_gn3d_cluster_mode"}       # the recorder's closing check and a row's own cluster-mode switch


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


class Spec:
    """A row, built: inputs {name: fp32 CPU tensor} in the order fn takes them; diff / weights: the names that are differentiable /
    that are parameters; fn(ops, t) -> the outputs that carry a gradient (HIP); ref(t) -> the same in plain torch, in the dtype and
    on the device of t; G: a gradient per output; switches: ops attributes for the run; extras() -> further fp32 draws
    {quantity: tensor}; ymask: the elements of output 0 the fp64 suite compares (conv2d_c1_relu's ReLU kink), else None;
    context(ecm) -> a context manager around every run (ops.split_products, the GroupNorm cluster mode); expect: entry points the
    canonical run must call.  calls: the entry points of the last run."""

    def __init__(self, rid, inputs, diff, fn, ref, G, weights=(), switches=None, extras=None, ymask=None, context=None, expect=()):
        self.rid, self.inputs, self.diff, self.fn, self.ref, self.G = rid, inputs, tuple(diff), fn, ref, tuple(G)
        self.weights, self.switches, self.extras, self.ymask = tuple(weights), switches or {}, extras, ymask
        self.context, self.expect, self.calls = context, set(expect), []


@contextlib.contextmanager
def switched(ecm, spec):
    prev = {k: getattr(ecm.ops, k) for k in spec.switches}
    for k, v in spec.switches.items():
        setattr(ecm.ops, k, v)
    try:
        with (spec.context(ecm) if spec.context else contextlib.nullcontext()):
            yield
    finally:
        for k, v in prev.items():
            setattr(ecm.ops, k, v)


# ---- layouts: views of equal values, each differentiable so that a weight can also be a non-leaf ---------------------------------------
def lay_reversed(t):
    p = tuple(reversed(range(t.dim())))
    return t.permute(p).contiguous().permute(p)                      # (the reversal is its own inverse)


def lay_channels_last(t):
    return t.contiguous(memory_format=torch.channels_last if t.dim() == 4 else torch.channels_last_3d)


def lay_off4(t):
    """One element into a larger buffer: data_ptr() % 16 == 4."""
    v = torch.cat([t.new_zeros(1), t.reshape(-1), t.new_zeros(3)])[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


def lay_step2(t):
    """Every second element of a buffer twice as wide in the last axis."""
    if t.dim() == 0:
        return torch.stack([t, t + 1.0])[0]
    v = torch.stack([t, t + 1.0], -1).flatten(-2)[..., ::2]
    assert v.shape == t.shape and (t.shape[-1] == 1 or v.stride(-1) == 2)
    return v


def layouts_of(t):
    out = {}
    if t.dim() >= 2 and not lay_reversed(t).is_contiguous():
        out["reversed"] = lay_reversed
    if t.dim() in (4, 5) and not lay_channels_last(t).is_contiguous():
        out["channels_last"] = lay_channels_last
    out["off4"] = lay_off4
    if t.numel() > 1:
        out["step2"] = lay_step2
    return out


# ---- one run ----------------------------------------------------------------------------------------------------------------------------
def execute(ecm, spec, need=None, place=None, nonleaf=(), G=None, gplace=None, use=None, label="canonical", into_grad=False):
    """Run spec.fn on the device: `need` = the inputs that require a gradient (default: all differentiable ones), place = {input:
    layout}, nonleaf = the inputs that are views of the leaf (the gradient is then the leaf's), G / gplace = the output gradients and
    their layout, use = the indices of the outputs that are used; into_grad: backward() into the leaves' .grad (AccumulateGrad runs)
    instead of autograd.grad.  -> {"y<i>": output, "g.<input>": gradient or None}."""
    ops = ecm.ops
    need = spec.diff if need is None else tuple(need)
    place, G = place or {}, spec.G if G is None else G
    leaves, t = {}, {}
    for k, v in spec.inputs.items():
        d = v.to(DEV)
        lay = place.get(k)
        if k in nonleaf:
            leaves[k] = d.requires_grad_(k in need)
            t[k] = (lay or (lambda a: a.view_as(a)))(leaves[k])
        else:
            if lay is not None:
                d = lay(d).detach()
                assert torch.equal(d, v.to(DEV))
            leaves[k] = t[k] = d.requires_grad_(k in need)
    with recording(ecm, f"{spec.rid}:{label}", census=False, strict=True) as calls, switched(ecm, spec), torch.enable_grad():
        ys = spec.fn(ops, t)
        ys = ys if isinstance(ys, tuple) else (ys,)
        use = [i for i in (range(len(ys)) if use is None else use) if ys[i].requires_grad]      # (x frozen: x[:head] carries nothing)
        gs = []
        for i in use:
            g = G[i].to(DEV)
            if gplace is not None:
                g = gplace(g).detach()
                assert torch.equal(g, G[i].to(DEV))
            gs.append(g)
        if into_grad:
            torch.autograd.backward([ys[i] for i in use], gs)
            ops.join_side_streams()
            grads = [leaves[k].grad for k in need]
        else:
            grads = torch.autograd.grad([ys[i] for i in use], [leaves[k] for k in need], gs, allow_unused=True) if need else ()
            ops.join_side_streams()
        torch.cuda.synchronize()
    spec.calls = [c for c in calls if c not in OWN_CALLS]
    assert set(calls) - OWN_CALLS or spec.rid.startswith("fork"), "no entry point was called"     # (one gradient: no sum)
    out = {f"y{i}": y.detach().clone() for i, y in enumerate(ys)}
    out.update({f"g.{k}": None for k in spec.diff})
    out.update({f"g.{k}": g for k, g in zip(need, grads)})
    for k in spec.diff:
        assert into_grad or leaves[k].grad is None
    for k, g in out.items():
        if g is not None and k.startswith("g."):
            assert g.shape == spec.inputs[k[2:]].shape and g.dtype == torch.float32, k
    return out


def same(a, b, keys, what, fails):
    for k in keys:
        if (a[k] is None) != (b[k] is None):
            fails.append(f"{what}: {k} is {'None' if b[k] is None else 'a tensor'}, canonical {'None' if a[k] is None else 'a tensor'}")
        elif a[k] is not None and not torch.equal(a[k], b[k]):
            bad = a[k] != b[k]
            fails.append(f"{what}: {k} differs from the canonical run in {int(bad.sum())} of {bad.numel()} elements "
                         f"(max |d| {float((a[k] - b[k]).abs().max()):.3e})")


def outputs(r):
    return [k for k in r if k.startswith("y")]


_SPECS, _CANON, _CALLS = {}, {}, {}


def spec_of(rid):
    if rid not in _SPECS:
        row = ROWS[rid]
        _SPECS[rid] = BUILDERS[row.kind](rid, row.case, **row.opts)
    return _SPECS[rid]


def canonical(ecm, rid):
    """The canonical run of a row, once per session (never written to afterwards)."""
    if rid not in _CANON:
        _CANON[rid] = execute(ecm, spec_of(rid))
        _CALLS[rid] = list(spec_of(rid).calls)
    return _CANON[rid]


# ---- builders -----------------------------------------------------------------------------------------------------------------------------
def _base(rid):
    """The name a row's operands are seeded under: a row and its fork=True / head=1 twin share them."""
    for tail in (".fork", ".head0", ".head1"):
        if rid.endswith(tail):
            return rid[:-len(tail)]
    return rid


def _he(name, *shape, fan):
    return seeded(name, *shape) * (2.0 / fan) ** 0.5


def build_conv3d(rid, case, fork=None):
    c = C3.CASES[case]
    fork = c.fork if fork is None else fork
    c = c._replace(fork=fork)
    o = tuple(2 * d for d in c.dims) if c.op == "deconv" else C3.out_dims(c.dims, c.stride)
    n = _base(rid)
    x = seeded(n + ".x", c.B, c.Ci, *c.dims)
    w = _he(n + ".w", *((c.Ci, c.Co) if c.op == "deconv" else (c.Co, c.Ci)), 3, 3, 3, fan=27 * c.Ci)
    G = [seeded(n + ".G", c.B, c.Co, *o)] + ([seeded(n + ".Gs", *x.shape)] if fork else [])
    if c.op == "deconv":
        fn = lambda ops, t: ops.deconv3d_k3s2(t["x"], t["w"])                                    # noqa: E731
        ref = lambda t: F.conv_transpose3d(t["x"], t["w"], None, 2, 1, 1)                        # noqa: E731
    else:
        fn = lambda ops, t: ops.conv3d_k3(t["x"], t["w"], c.stride, fork=fork)                   # noqa: E731
        ref = lambda t: (F.conv3d(t["x"], t["w"], None, c.stride, 1),) + ((t["x"],) if fork else ())       # noqa: E731

    def extras():
        Gs = G[1] if fork else None
        names = {"y": "y0", "gx": "g.x", "gw": "g.w"}
        draws = [C3._chain32(c, C3.launches(c), x, w, G[0], Gs)]
        # the Winograd restatement as the fp64 suite admits it: y and gx on a Winograd row, gw where the Winograd weight gradient
        # is the path taken (WINOGRAD_WGRAD is pinned on below) -- which is the same rows
        if c.op == "conv" and c.stride == 1 and C3.wino_ok(c.dims, c.wino) and not C3.is_c1(c.Co, c.Ci, c.stride):
            draws.append(C3._wino32(c, x, w, G[0], Gs))
        return [{names[k]: v for k, v in d.items()} for d in draws]
    return Spec(rid, {"x": x, "w": w}, ("x", "w"), fn, ref, G, weights=("w",), switches={"WINOGRAD": c.wino, "WINOGRAD_WGRAD": True}, extras=extras)


def build_split(rid, case, fork):
    """ops.conv3d_k3 at stride 2 inside ops.split_products("bf16x3"): forward and data gradient on the split-bf16 kernels."""
    B, Ci, Co, dims, odims, _ = SPC.CONV_CASES[case]
    n = _base(rid)
    x, w = seeded(n + ".x", B, Ci, *dims), _he(n + ".w", Co, Ci, 3, 3, 3, fan=27 * Ci)
    G = [seeded(n + ".G", B, Co, *odims)] + ([seeded(n + ".Gs", *x.shape)] if fork else [])
    return Spec(rid, {"x": x, "w": w}, ("x", "w"), lambda ops, t: ops.conv3d_k3(t["x"], t["w"], 2, fork=fork),
                lambda t: (F.conv3d(t["x"], t["w"], None, 2, 1),) + ((t["x"],) if fork else ()), G, weights=("w",),
                extras=lambda: [{"y0": SP.chain_conv(x.to(DEV), w.to(DEV), 2, 2)}],
                context=lambda ecm: ecm.ops.split_products("bf16x3", SP.ALL), expect=SP.SPLIT_SYMS)


def build_conv2d(rid, case, fork=False):
    c = C2.CASES[case]._replace(fork=fork)
    o = C2.operands(case, c)                      # (the fp64 suite's operands: conv2d_c1_relu's G is masked at the ReLU's kink there)
    inputs = {k: o[k] for k in ("x", "w", "b") if o[k] is not None}
    G = [o["G"]] + ([o["Gs"]] if fork else [])
    if c.op == "c1":
        fn = lambda ops, t: ops.conv2d_c1_relu(t["x"], t["w"], t["b"])                            # noqa: E731
    elif c.op == "deconvb":
        fn = lambda ops, t: ops.deconv2d_k3s2_bias(t["x"], t["w"], t["b"])                        # noqa: E731
    elif c.op == "planes":
        fn = lambda ops, t: ops.conv2d_planes(t["x"], t["w"], fork=fork)                          # noqa: E731
    elif c.cls is not None:
        assert not fork
        fn = lambda ops, t: ops.conv2d(t["x"], t["w"], 1, 1, *C2.geometry(c))                     # noqa: E731
    else:
        fn = lambda ops, t: ops.conv2d(t["x"], t["w"], c.stride, c.dil, fork=fork)                # noqa: E731
    ref = lambda t: (C2._forward(c, t["x"], t["w"], t.get("b")),) + ((t["x"],) if fork else ())   # noqa: E731

    def extras():
        names = {"y": "y0", "gx": "g.x", "gw": "g.w"}
        L = C2.launches(c)
        wq = {q for q, fam, _ in L if fam in ("wino", "wgw")}
        draws = [C2._chain32(c, o, L)] + ([C2._wino32(c, o, wq)] if wq else [])
        return [{names[k]: v for k, v in d.items()} for d in draws]
    sw = {"WINOGRAD": c.wino, "WINOGRAD_WGRAD": c.ww}
    if c.min_ci is not None:
        sw["WINO2D_MIN_CI"] = c.min_ci
    keep = o.get("keep")
    return Spec(rid, inputs, tuple(inputs), fn, ref, G, weights=tuple(k for k in inputs if k != "x"), switches=sw, extras=extras,
                ymask=None if keep is None else keep.double())


def build_gn(rid, case, skip, relu, head, mode=1):
    shape, n = (2,) + tuple(GN.CASES[case][1:]), _base(rid)
    x = seeded(n + ".x", *shape) * 1.7 + 0.3
    inputs = {"x": x, "gamma": 1 + 0.2 * seeded(n + ".gamma", shape[1]), "beta": 0.2 * seeded(n + ".beta", shape[1])}
    if skip:
        inputs["skip"] = seeded(n + ".skip", *shape)

    def pre(t):
        p = F.group_norm(t["x"], GN.GROUPS, t["gamma"], t["beta"], GN.EPS)
        return p + t["skip"] if skip else p
    G0 = seeded(n + ".G", *shape)
    if relu:                                      # the fp64 suite's tie rule: no gradient through a pre-activation within TIE of 0
        tie = pre({k: v.double() for k, v in inputs.items()}).abs() < GN.TIE
        assert float(tie.float().mean()) <= GN.TIE_SHARE
        G0 = G0.masked_fill(tie, 0.0)
    G = [G0] + ([seeded(n + ".Gh", head, *shape[1:])] if head else [])
    fn = lambda ops, t: ops.group_norm_act(t["x"], t["gamma"], t["beta"], t.get("skip"), relu=relu, head=head)     # noqa: E731
    ref = lambda t: ((F.relu(pre(t)) if relu else pre(t)),) + ((t["x"][:head],) if head else ())                  # noqa: E731
    return Spec(rid, inputs, tuple(inputs), fn, ref, G, weights=("gamma", "beta"),
                context=None if mode == 1 else (lambda ecm: GN.cluster_mode(ecm, mode)))


def build_tail(rid, shape):
    inputs = {"x": seeded(rid + ".x", *shape) * 1.7 + 0.3, "gamma": 1 + 0.2 * seeded(rid + ".gamma", 32),
              "beta": 0.2 * seeded(rid + ".beta", 32), "w": _he(rid + ".w", 1, 32, 3, 3, 3, fan=27 * 32)}
    pre = lambda t: F.group_norm(t["x"], 32, t["gamma"], t["beta"], GN.EPS)                       # noqa: E731
    tie = pre({k: v.double() for k, v in inputs.items()}).abs() < GN.TIE
    assert not bool(tie.any()), "a pre-activation of the classifier tail's row lies at the ReLU's kink: reseed"
    fn = lambda ops, t: ops.classifier_tail(t["x"], t["gamma"], t["beta"], t["w"])                # noqa: E731
    ref = lambda t: F.conv3d(F.relu(pre(t)), t["w"], None, 1, 1)                                  # noqa: E731
    return Spec(rid, inputs, tuple(inputs), fn, ref, [seeded(rid + ".G", shape[0], 1, *shape[2:])], weights=("gamma", "beta", "w"))


def build_costvol(rid, shape):
    B, Cc, h, w, D = shape
    inputs = {"left": seeded(rid + ".L", B, Cc, h, w), "right": seeded(rid + ".R", B, Cc, h, w)}
    return Spec(rid, inputs, tuple(inputs), lambda ops, t: ops.cost_volume(t["left"], t["right"], D),
                lambda t: CG.cost_volume_t(t["left"], t["right"], D), [seeded(rid + ".G", B, 2 * Cc, D, h, w)])


def build_costvol_conv(rid, case):
    c = CG.WHOLE[case]
    assert case != "cc_w1" or c == min(CG.WHOLE.values(), key=lambda c: c.B * c.h * c.w * c.D)
    inputs = {"left": seeded(rid + ".L", c.B, 32, c.h, c.w), "right": seeded(rid + ".R", c.B, 32, c.h, c.w),
              "weight": _he(rid + ".W", 32, 64, 3, 3, 3, fan=27 * 64)}
    return Spec(rid, inputs, tuple(inputs), lambda ops, t: ops.costvol_conv3d(t["left"], t["right"], t["weight"], c.D),
                lambda t: CG.collapsed_t(t["left"], t["right"], t["weight"], c.D), [seeded(rid + ".G", c.B, 32, c.D, c.h, c.w)],
                weights=("weight",))


def build_context(rid, table, variant=None):
    cases = {n: c for n, c in getattr(CM, table).items() if variant is None or (c.variant == variant and c.grads)}
    name = min(cases, key=lambda n: max(t.numel() for t in CM.operands(n).values()))
    c, o = cases[name], CM.operands(name)
    inputs = {k: o[k] for k in CM.INPUTS[type(c)]}
    if isinstance(c, CM.WCase):
        fn = lambda ops, t: ops.context_weights(*t.values(), c.variant)                           # noqa: E731
        ref = lambda t: CM.planes_t(*t.values(), c.variant)                                       # noqa: E731
    elif isinstance(c, CM.SCase):
        fn = lambda ops, t: ops.softargmin_heads(t["c"])                                          # noqa: E731
        ref = lambda t: CM._heads(soft_argmin_t, t["c"], c.NH)                                    # noqa: E731
    elif isinstance(c, CM.ACase):
        fn = lambda ops, t: ops.ecm_aggregate9(t["d"], t["w9"], c.s)                              # noqa: E731
        ref = lambda t: CM.aggregate9_t(t["d"], t["w9"], c.s)                                     # noqa: E731
    elif isinstance(c, CM.VCase):
        fn = lambda ops, t: ops.volume_mapping(t["c"], t["m5"], t["mt3"], c.s)                    # noqa: E731
        ref = lambda t: CM._heads(lambda u: volume_mapping_t(u, t["m5"], t["mt3"], c.s), t["c"], c.NH)     # noqa: E731
    else:
        fn = lambda ops, t: ops.trilinear_softargmin(t["c"], c.Do, c.H, c.W)                      # noqa: E731
        ref = lambda t: CM._heads(lambda u: trilinear_t(u, c.Do, c.H, c.W), t["c"], c.NH)         # noqa: E731
    return Spec(rid, inputs, tuple(inputs), fn, ref, [o["G"]], weights=tuple(k for k in inputs if k.startswith("W")))


LOSS_WEIGHTS = (0.5, 0.7, 1.0)


def build_loss(rid, shape):
    n = 1
    for s in shape:
        n *= s
    gt, p1, p2, p3 = CG.loss_table(n)
    inputs = {"p1": p1.view(shape), "p2": p2.view(shape), "p3": p3.view(shape), "gt": gt.view(shape[0], *shape[2:])}
    fn = lambda ops, t: ops.stereo_loss3([t["p1"], t["p2"], t["p3"]], t["gt"], CG.MAXDISP, LOSS_WEIGHTS)[0]        # noqa: E731
    ref = lambda t: O.train_loss([t[k].reshape(1, 1, -1) for k in ("p1", "p2", "p3")], t["gt"].reshape(1, -1))  # noqa: E731
    return Spec(rid, inputs, ("p1", "p2", "p3"), fn, ref, [torch.ones(())])


def build_fork(rid, shape, n):
    inputs = {"x": seeded(rid + ".x", *shape)}
    return Spec(rid, inputs, ("x",), lambda ops, t: ops.fork(t["x"], n), lambda t: (t["x"],) * n,
                [seeded(f"{rid}.G{i}", *shape) for i in range(n)])


def build_fork_head(rid, shape, n):
    inputs = {"x": seeded(rid + ".x", *shape)}
    return Spec(rid, inputs, ("x",), lambda ops, t: ops.fork_head(t["x"], n), lambda t: (t["x"], t["x"][:n]),
                [seeded(rid + ".G", *shape), seeded(rid + ".Gh", n, *shape[1:])])


BUILDERS = {"conv3d": build_conv3d, "conv2d": build_conv2d, "gn": build_gn, "tail": build_tail, "costvol": build_costvol,
            "costvol_conv": build_costvol_conv, "split": build_split, "context": build_context, "loss": build_loss, "fork": build_fork,
            "fork_head": build_fork_head}
ALL = sorted(ROWS)


# ---- the canonical run against fp64 ---------------------------------------------------------------------------------------------------------
def torch_run(spec, dtype, device):
    t = {k: v.to(device=device, dtype=dtype, copy=True).requires_grad_(k in spec.diff) for k, v in spec.inputs.items()}
    ys = spec.ref(t)
    ys = ys if isinstance(ys, tuple) else (ys,)
    grads = torch.autograd.grad(ys, [t[k] for k in spec.diff], [g.to(device=device, dtype=dtype) for g in spec.G])
    out = {f"y{i}": y.detach() for i, y in enumerate(ys)}
    out.update({f"g.{k}": g for k, g in zip(spec.diff, grads)})
    return out


@pytest.mark.parametrize("rid", ALL)
def test_canonical_run_against_fp64(ecm, rid):
    spec, a = spec_of(rid), canonical(ecm, rid)
    assert spec.expect <= set(_CALLS[rid]), f"the canonical run called {sorted(set(_CALLS[rid]))}, not {sorted(spec.expect)}"
    q64 = torch_run(spec, torch.float64, "cpu")
    draws = [torch_run(spec, torch.float32, "cpu"), torch_run(spec, torch.float32, DEV)] + (spec.extras() if spec.extras else [])
    assert set(a) == set(q64)
    fails = []
    for k, got in a.items():
        ref = q64[k]
        assert got is not None and got.shape == ref.shape, k
        mask = spec.ymask if (k == "y0" and spec.ymask is not None) else 1.0
        each = [float(((d[k].cpu().double() - ref).abs() * mask).max()) for d in draws if k in d]
        e32, scale = max(each), float((ref * mask).abs().max())
        err = float(((got.cpu().double() - ref).abs() * mask).max())
        bound = K * e32 + FLOOR * scale
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"ACRATIO {rid} {k} {ratio:.3f}   # err {err:.3e}, e32 {e32:.3e} [{' '.join('%.2e' % e for e in each)}], max|ref| {scale:.3e}")
        if not err <= bound:
            fails.append(f"{rid}: {k}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")
    b = execute(ecm, spec, label="repeat")
    same(a, b, list(a), "a second canonical run", fails)
    assert not fails, "\n".join(fails)


# ---- V1: gradient subsets ----------------------------------------------------------------------------------------------------------------
def subsets_of(rid, diff):
    if "ContextWeights" in ROWS[rid].functions:
        return list(CONTEXT_SUBSETS)
    return [s for r in range(1, len(diff)) for s in itertools.combinations(diff, r)]


def data_launches(calls):
    """The launches of a convolution row that are its forward or its data gradient: neither a pack, a size query, a weight or
    bias gradient."""
    return [c for c in calls if not any(s in c for s in ("pack", "scratch", "bytes", "floats", "wgrad", "channel_sum"))]


ONE_INPUT = ("softargmin_heads", "trilinear_softargmin")          # and the forks: one differentiable input, no proper subset


@pytest.mark.parametrize("rid", [r for r in ALL if r not in ONE_INPUT and ROWS[r].kind not in ("fork", "fork_head")])
def test_v1_gradient_subsets(ecm, rid):
    spec, a = spec_of(rid), canonical(ecm, rid)
    subsets = subsets_of(rid, spec.diff)
    assert subsets
    fails = []
    full = data_launches(_CALLS[rid])
    for need in subsets:
        b = execute(ecm, spec, need=need, label="needs " + "+".join(need))
        if ROWS[rid].kind in ("conv3d", "conv2d", "split"):      # what a frozen operand's gradient alone needed is not launched
            if not {"w", "b"} & set(need) and any("wgrad" in c for c in spec.calls):
                fails.append(f"needs {need}: launched {[c for c in spec.calls if 'wgrad' in c]}")
            if "x" not in need and not len(data_launches(spec.calls)) < len(full):
                fails.append(f"needs {need}: as many forward / data-gradient launches as the canonical run, {data_launches(spec.calls)}")
        for k in spec.diff:
            if k not in need and b[f"g.{k}"] is not None:
                fails.append(f"needs {need}: a gradient for {k}")
        same(a, b, outputs(a) + [f"g.{k}" for k in need], f"needs {need}", fails)
    assert not fails, "\n".join(fails)


# ---- V2: operand layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ALL)
def test_v2_operand_layouts(ecm, rid):
    spec, a = spec_of(rid), canonical(ecm, rid)
    fails = []
    for k, v in spec.inputs.items():
        for lname, lay in layouts_of(v).items():
            for nonleaf in ((False, True) if k in spec.weights else (False,)):
                what = f"{k} as {lname}" + (" (non-leaf)" if nonleaf else "")
                b = execute(ecm, spec, place={k: lay}, nonleaf=(k,) if nonleaf else (), label=what)
                same(a, b, list(a), what, fails)
    for k in spec.weights:                        # a contiguous weight that is a view of its leaf (nn.DataParallel's replicas)
        b = execute(ecm, spec, nonleaf=(k,), label=f"{k} non-leaf")
        same(a, b, list(a), f"{k} as a non-leaf view", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rid", OVERLAP_ROWS)
def test_v2_weight_layouts_beside_the_side_stream(ecm, rid):
    """The weight's layouts again with ops.enable_wgrad_overlap(True) and backward() into .grad: a contiguous leaf's gradient is
    launched on the side stream, any other weight's must stay on the main stream (ctx.side_ok, ops._on_side) because
    AccumulateGrad re-lays it out there at once."""
    spec, a, ops = spec_of(rid), canonical(ecm, rid), ecm.ops
    fails = []
    prev = ops.enable_wgrad_overlap(True)
    try:
        for lname, lay in [("contiguous", None)] + list(layouts_of(spec.inputs["w"]).items()):
            for nonleaf in (False, True):
                what = f"w as {lname}" + (" (non-leaf)" if nonleaf else "") + ", overlap on"
                b = execute(ecm, spec, place={} if lay is None else {"w": lay}, nonleaf=("w",) if nonleaf else (), label=what,
                            into_grad=True)
                same(a, b, list(a), what, fails)
    finally:
        ops.enable_wgrad_overlap(prev)
        ops.join_side_streams()
    assert not fails, "\n".join(fails)


# ---- V3: gradient layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ALL)
def test_v3_gradient_layouts(ecm, rid):
    spec, a = spec_of(rid), canonical(ecm, rid)
    fails = []
    for lname, lay in layouts_of(max(spec.G, key=lambda g: g.dim())).items():
        if any(g.dim() not in (4, 5) for g in spec.G) and lname == "channels_last":
            continue
        b = execute(ecm, spec, gplace=lay, label="G as " + lname)
        same(a, b, list(a), "G as " + lname, fails)
    if all(g.dim() >= 3 for g in spec.G):         # what y.sum().backward() hands over: a stride-0 expand of a [B,C,1,...] tensor
        small = [g[(slice(None), slice(None)) + (slice(0, 1),) * (g.dim() - 2)].contiguous() for g in spec.G]
        dense = [s.expand(g.shape).contiguous() for s, g in zip(small, spec.G)]
        c = execute(ecm, spec, G=dense, label="G dense copy of the expand")
        b = execute(ecm, spec, G=dense, gplace=lambda g: g[(slice(None), slice(None)) + (slice(0, 1),) * (g.dim() - 2)].expand(g.shape),
                    label="G as a stride-0 expand")
        same(c, b, list(c), "G as a stride-0 expand", fails)
    assert not fails, "\n".join(fails)


# ---- V4: unused outputs ------------------------------------------------------------------------------------------------------------------
FORK_ROWS = [r for r in ALL if ROWS[r].opts.get("fork")]


@pytest.mark.parametrize("rid", FORK_ROWS)
def test_v4_convolution_fork_outputs(ecm, rid):
    spec, a = spec_of(rid), canonical(ecm, rid)
    plain = canonical(ecm, rid[:-len(".fork")])
    fails = []
    b = execute(ecm, spec, use=[0], label="y only")
    same(plain, b, ["y0", "g.x", "g.w"], "used through y only, against fork=False", fails)
    b = execute(ecm, spec, use=[1], label="skip only")
    if b["g.w"] is not None:
        fails.append("used through the skip only: the weight has a gradient")
    if b["g.x"] is None or not torch.equal(b["g.x"], spec.G[1].to(DEV)):
        fails.append("used through the skip only: gx is not the skip gradient")
    b = execute(ecm, spec, use=[0, 1], label="both")
    same(a, b, list(a), "used through both", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rid", [r for r in ALL if ROWS[r].kind == "fork"])
def test_v4_fork_output_subsets(ecm, rid):
    spec = spec_of(rid)
    n, fails = len(spec.G), []
    for r in range(1, n + 1):
        for use in itertools.combinations(range(n), r):
            b = execute(ecm, spec, use=list(use), label=f"outputs {use}")
            want = spec.G[use[0]].to(DEV)
            for i in use[1:]:
                want = want + spec.G[i].to(DEV)
            if not torch.equal(b["g.x"], want):
                fails.append(f"outputs {use}: gx is not ((g0 + g1) + g2) + ... over the gradients present")
    assert not fails, "\n".join(fails)


HEAD_ROWS = [r for r in ALL if ROWS[r].kind == "fork_head" or ROWS[r].opts.get("head")]


@pytest.mark.parametrize("rid", HEAD_ROWS)
def test_v4_head_fork_outputs(ecm, rid):
    spec, a = spec_of(rid), canonical(ecm, rid)
    fails = []
    b = execute(ecm, spec, use=[0], label="full only")
    if ROWS[rid].kind == "fork_head":
        if not torch.equal(b["g.x"], spec.G[0].to(DEV)):
            fails.append("full only: gx is not the full gradient")
    else:
        same(canonical(ecm, rid[:-1] + "0"), b, ["y0"] + [f"g.{k}" for k in spec.diff], "full only, against head=0", fails)
    b = execute(ecm, spec, use=[0, 1], label="full + head")
    same(a, b, list(a), "full + head", fails)
    with pytest.raises(RuntimeError, match="produced no gradient"):
        execute(ecm, spec, use=[1], label="head only")
    b = execute(ecm, spec, label="after the refusal")                  # the device takes work afterwards
    same(a, b, list(a), "after the refused head-only pass", fails)
    ecm.ops.check_async_errors()
    assert not fails, "\n".join(fails)


def test_v4_stereo_loss3_scaled_and_with_metrics(ecm):
    """backward of 2.0 * loss: every gradient exactly twice the canonical one (a power-of-two scale is exact wherever it is applied);
    the metrics output used alongside changes nothing."""
    spec, a = spec_of("stereo_loss3"), canonical(ecm, "stereo_loss3")
    b = execute(ecm, spec, G=[torch.full((), 2.0)], label="2 * loss")
    for k in spec.diff:
        assert torch.equal(b[f"g.{k}"], 2.0 * a[f"g.{k}"]), k
    ops = ecm.ops
    t = {k: v.to(DEV).requires_grad_(k in spec.diff) for k, v in spec.inputs.items()}
    with recording(ecm, "stereo_loss3:metrics", census=False, strict=True):
        loss, met = ops.stereo_loss3([t["p1"], t["p2"], t["p3"]], t["gt"], CG.MAXDISP, LOSS_WEIGHTS)
        assert not met.requires_grad
        (2.0 * loss + met[2].detach() + met.sum() * 0.0).backward()
    for k in spec.diff:
        assert torch.equal(t[k].grad, 2.0 * a[f"g.{k}"]), k
    assert torch.equal(loss.detach(), a["y0"]) and float(met[0]) == float(loss)


# ---- V5: accumulation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True], ids=["main", "overlap"])
@pytest.mark.parametrize("rid", ACCUMULATION_ROWS)
def test_v5_weight_gradient_accumulation(ecm, rid, overlap):
    spec, ops = spec_of(rid), ecm.ops
    G2 = [g.flip(-1).contiguous() * 0.5 for g in spec.G]
    ga, gb = canonical(ecm, rid)["g.w"], execute(ecm, spec, G=G2, label="second gradient")["g.w"]
    want = ga + gb
    prev = ops.enable_wgrad_overlap(overlap)
    try:
        for mode in ("two calls in one graph", "two backward passes"):
            t = {k: v.to(DEV).requires_grad_(k in spec.diff) for k, v in spec.inputs.items()}
            with recording(ecm, f"{rid}:{mode}", census=False, strict=True), switched(ecm, spec), torch.enable_grad():
                if mode == "two calls in one graph":
                    torch.autograd.backward([spec.fn(ops, t), spec.fn(ops, t)], [spec.G[0].to(DEV), G2[0].to(DEV)])
                else:
                    spec.fn(ops, t).backward(spec.G[0].to(DEV))
                    spec.fn(ops, t).backward(G2[0].to(DEV))
                ops.join_side_streams()
                torch.cuda.synchronize()
            assert torch.equal(t["w"].grad, want), f"{mode}: w.grad is not the fp32 sum of the two single-call gradients"
    finally:
        ops.enable_wgrad_overlap(prev)
        ops.join_side_streams()


# ---- V6: refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ALL)
def test_v6_refusals(ecm, rid):
    spec, ops = spec_of(rid), ecm.ops
    fails = []
    for k in spec.inputs:
        for what, conv in (("float64", lambda v: v.to(DEV).double()), ("float16", lambda v: v.to(DEV).half()), ("cpu", lambda v: v.clone())):
            t = {n: (conv(v) if n == k else v.to(DEV)).requires_grad_(n in spec.diff) for n, v in spec.inputs.items()}
            with recording(ecm, f"{rid}:{k} {what}", census=False, strict=True) as calls, switched(ecm, spec), torch.enable_grad():
                try:
                    spec.fn(ops, t)
                    fails.append(f"{k} as {what}: accepted")
                except RuntimeError:
                    pass
            made = [c for c in calls if c not in OWN_CALLS]
            if made:
                fails.append(f"{k} as {what}: refused after {made}")
    assert not fails, "\n".join(fails)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["cmfsm", "cmf"])
def test_model_frozen_parts(ecm, arch):
    """One stereo_loss3 training step at 256 x 256, batch 1, with everything trainable, with feature_extraction frozen and with
    everything but feature_extraction frozen: a frozen parameter has no gradient, every other gradient is bit-identical to the
    all-trainable step's, and no slow path is taken."""
    ops, models = ecm.ops, ecm.models
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(11)
    left, right = torch.randn(1, 3, 256, 256, device=DEV, generator=gen), torch.randn(1, 3, 256, 256, device=DEV, generator=gen)
    gt = (torch.rand(1, 256, 256, generator=torch.Generator().manual_seed(8)) * 191.0).to(DEV)
    encoder = {n for n, _ in model.named_parameters() if n.startswith("feature_extraction.")}
    assert encoder and len(encoder) < len(list(model.parameters()))
    models.SLOW_PATH_EVENTS.clear()

    def step(frozen):
        for n, p in model.named_parameters():
            p.requires_grad_(n not in frozen)
        model.zero_grad(set_to_none=True)
        with recording(ecm, f"{arch}:frozen {len(frozen)}", census=False, strict=True), torch.enable_grad():
            loss, _ = ops.stereo_loss3(model(left, right), gt, 192)
            loss.backward()
            ops.join_side_streams()
            torch.cuda.synchronize()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}, loss.detach().clone()

    everyone = {n for n, _ in model.named_parameters()}
    full, loss = step(set())
    assert all(g is not None for g in full.values())
    fails = []
    for what, frozen in (("feature_extraction frozen", encoder), ("all but feature_extraction frozen", everyone - encoder)):
        got, l2 = step(frozen)
        if not torch.equal(l2, loss):
            fails.append(f"{what}: the loss moved")
        for n, g in got.items():
            if n in frozen:
                if g is not None:
                    fails.append(f"{what}: {n} is frozen and has a gradient")
            elif g is None or not torch.equal(g, full[n]):
                fails.append(f"{what}: the gradient of {n} is {'missing' if g is None else 'not bit-identical to the all-trainable step'}")
    for p in model.parameters():
        p.requires_grad_(True)
    assert not models.SLOW_PATH_EVENTS, models.SLOW_PATH_EVENTS
    assert not fails, f"{len(fails)} failures, the first 20:\n" + "\n".join(fails[:20])
