"""GroupNorm forward AND backward against fp64, on every kernel path of csrc/gn3d.hip.

Three implementations compute the same arithmetic -- the cluster kernels (gn_fused_fwd / gn_fused_bwd), the two-stage fp32
kernels and the bf16 instantiations of the two-stage templates -- and which one runs is decided silently by shape and mode
(`fused_geom`, `ecm_gn3d_cluster_mode`, graph capture).  The case table below names, for every path and every edge inside a
path, a shape that reaches it; `fused_geom` is restated here in Python so that the mapping is asserted (tests/test_gn_geometry.py
on the CPU with 512 resident workgroups, `test_case_table_covers_every_class_on_this_device` with the real CU count) instead of
assumed.

Yardstick (the one of test_hip_numerics.py, extended to the gradients).  Reference: F.group_norm in fp64 on the device, `+ skip`
and `relu` written out, gradients from autograd.  Unit: the reference's OWN fp32 error -- the same expression evaluated by torch
in fp32 on the device and on the CPU (two independent summation orders; the device alone from 1 GB of operands up),
e32(q) = max |q32 - q64|.  A kernel passes when  |q_hip - q64|_max <= K * e32(q) + FLOOR * max|q64|  with K = 4, FLOOR = 2e-7.
The residual operand's gradient is a (masked) copy of gy and must EQUAL the fp64 reference cast to fp32.

ReLU ties: an element whose pre-activation is within rounding of 0 may be masked differently in fp32 and fp64, which changes g
there and, through sum g / sum g*xhat, every element of the group.  No element is excluded from any comparison; instead the
incoming gradient is set to 0 wherever the fp64 pre-activation is below 1e-4 in magnitude (pre-activations are of order 1 and
their fp32 rounding near 1e-6), so the mask decision there has no effect on any output.  The zeroed share is asserted <= 1e-3.

Every case runs twice on fresh operands in each mode and must reproduce bit for bit: the ticket scheme makes the ASSIGNMENT of
work non-deterministic, only the fixed-order reductions make the results deterministic.  Operands differ between cases, and all
outputs of a case stay alive until it ends, so an element a kernel failed to write cannot inherit the right value from recycled
memory.

Each test prints `GNRATIO <path> <quantity> <ratio>` with ratio = |q_hip - q64| / (K * e32 + floor); DESIGN.md section 4 holds
the worst ratio per path as measured on the MI355X."""
import contextlib
import ctypes as C
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K, FLOOR = 4.0, 2e-7            # test_hip_numerics.py: 4 x torch's own fp32 error + one fp32 ulp of the output scale
TIE, TIE_SHARE = 1e-4, 1e-3
EPS = 1e-5
BIG_BYTES = 1 << 30             # x, skip, gy, y in fp32 from here up: the device's fp32 evaluation alone gives the unit

# ---- csrc/gn3d.hip: fused_geom, restated (tests/test_gn_geometry.py pins these constants to the source) ---------------------
GROUPS = 32
THREADS = 256
CHUNK = 32768
FWD_MAXV4, FWDS_MAXV4, BWD_MAXV4 = 32, 24, 20
FWD_OCC, BWD_OCC = 2, 2
FUSED_MAX_CPG = 8
FUSED_MAX_CL_RUN = 128
TWO_STAGE = "two-stage"


def fused_geom(B, C, S, maxv4, resident):
    """-> TWO_STAGE or (cpg, wpc, cl, grid, v4_per_wg): the cluster launch of a [B, C, S] tensor with `maxv4` float4 per thread."""
    if S % 4 != 0 or S // 4 >= 0x7fffffff - 0x10000 or C % GROUPS != 0 or resident <= 0:
        return TWO_STAGE
    cpg = C // GROUPS
    if cpg > FUSED_MAX_CPG:
        return TWO_STAGE
    nv4, cap = S // 4, THREADS * maxv4
    wpc = (nv4 + cap - 1) // cap
    if wpc * cpg > FUSED_MAX_CL_RUN or wpc * cpg * 4 > resident:
        return TWO_STAGE
    cl = wpc * cpg
    total = B * GROUPS * cl
    if total >= 0x7fffffff:
        return TWO_STAGE
    return cpg, wpc, cl, min(total, resident), (nv4 + wpc - 1) // wpc


def _bcs(shape):
    S = 1
    for d in shape[2:]:
        S *= d
    return shape[0], shape[1], S


def geoms(shape, cus):
    """The three cluster launches a shape can meet: forward, forward with a residual operand, backward."""
    B, C_, S = _bcs(shape)
    return {"fwd": fused_geom(B, C_, S, FWD_MAXV4, cus * FWD_OCC), "fwds": fused_geom(B, C_, S, FWDS_MAXV4, cus * FWD_OCC),
            "bwd": fused_geom(B, C_, S, BWD_MAXV4, cus * BWD_OCC)}


def chunks_of(n):
    return (n + CHUNK - 1) // CHUNK


# ---- the case table ------------------------------------------------------------------------------------------------------------
_P = 12289                      # a prime number of float4: every slice count > 1 leaves a ragged last slice
SMALL = {
    # cluster, one workgroup per channel: part of one wave; not a multiple of a wave; exactly THREADS * MAXV4 float4 for each
    # of the three MAXV4 and one float4 more (two workgroups, slices of MAXV4 * 128 + 1 and MAXV4 * 128 float4)
    "w1_part_wave": (2, 32, 4, 5, 10),
    "w1_ragged_wave": (1, 32, 10, 20, 20),
    "w1_full_fwd": (1, 32, 4 * THREADS * FWD_MAXV4), "w1_full_fwd_plus1": (1, 32, 4 * THREADS * FWD_MAXV4 + 4),
    "w1_full_fwds": (1, 32, 4 * THREADS * FWDS_MAXV4), "w1_full_fwds_plus1": (1, 32, 4 * THREADS * FWDS_MAXV4 + 4),
    "w1_full_bwd": (1, 32, 4 * THREADS * BWD_MAXV4), "w1_full_bwd_plus1": (1, 32, 4 * THREADS * BWD_MAXV4 + 4),
    # several workgroups per channel with a ragged last slice, 1 / 2 / 4 / 8 channels per group
    "ragged_cpg1": (1, 32, 4 * _P), "ragged_cpg2": (1, 64, 4 * _P), "ragged_cpg4": (1, 128, 4 * _P), "ragged_cpg8": (1, 256, 4 * _P),
    # more tickets than resident workgroups in all three launches: a workgroup's parked stores leave under its next ticket's
    # rendezvous, and a ragged last slice is followed by a full one
    "tickets": (5, 64, 4 * _P),
    # two-stage by shape: S % 4 = 1, 2, 3; ten channels per group (two chunks, vector loops)
    "s_mod4_1": (2, 64, 3, 5, 7), "s_mod4_2": (1, 32, 2, 3, 5), "s_mod4_3": (1, 32, 7, 9, 5), "cpg10": (1, 320, 40000),
    # two-stage chunking (mode 0): S and cpg * S around CHUNK, two channels per group, and one S % 4 != 0 above two chunks
    "chunk_m4": (1, 64, CHUNK - 4), "chunk_0": (1, 64, CHUNK), "chunk_p4": (1, 64, CHUNK + 4), "chunk_2p4": (1, 64, 2 * CHUNK + 4),
    "chunk_3m4": (1, 64, 3 * CHUNK - 4), "chunk_2p1_scalar": (1, 64, 2 * CHUNK + 1),
    # both branches of gn_pivot and its strides 1 and 2
    "pivot_n1": (2, 32, 1), "pivot_n2": (2, 32, 2), "pivot_n15": (2, 32, 15), "pivot_n16": (2, 32, 16), "pivot_n17": (2, 32, 17),
    "pivot_n31": (2, 32, 31), "pivot_n32": (2, 32, 32),
}
# forward on the cluster kernel, backward on the two-stage kernels reading the statistics the cluster kernel wrote
MIXED = {"mixed_band": (1, 32, 4 * (FUSED_MAX_CL_RUN * THREADS * BWD_MAXV4 + 3))}
# the shapes of the training step, and the 1080p volume that is two-stage in both directions (255 workgroups per channel)
PRODUCTION = {"prod_3d_32": (4, 32, 48, 144, 240), "prod_3d_64": (4, 64, 24, 72, 120), "prod_2d_128": (8, 128, 144, 240),
              "prod_2d_32": (8, 32, 576, 960), "prod_1080p": (1, 32, 64, 272, 480)}
CASES = {**SMALL, **MIXED, **PRODUCTION}
PIVOT_N = (1, 2, 15, 16, 17, 31, 32)
CHUNK_S = (CHUNK - 4, CHUNK, CHUNK + 4, 2 * CHUNK + 4, 3 * CHUNK - 4)


def missing_classes(cus):
    """The path classes (see the module docstring and the case table) that NO case reaches on a device of `cus` compute units."""
    G = {k: (_bcs(s), geoms(s, cus)) for k, s in CASES.items()}
    fused = lambda g: g != TWO_STAGE                                                    # noqa: E731
    launches = [(bcs, g, key) for bcs, gs in G.values() for key, g in gs.items() if fused(g)]
    maxv4 = {"fwd": FWD_MAXV4, "fwds": FWDS_MAXV4, "bwd": BWD_MAXV4}
    want = {"cluster wpc=1, part of one wave": any(g[1] == 1 and S // 4 < 64 for (_, _, S), g, _ in launches),
            "cluster wpc=1, ragged wave": any(g[1] == 1 and S // 4 > 64 and (S // 4) % 64 for (_, _, S), g, _ in launches)}
    for key, m in maxv4.items():
        want[f"cluster {key}: wpc=1 at exactly THREADS*MAXV4"] = any(k == key and g[1] == 1 and S // 4 == THREADS * m
                                                                     for (_, _, S), g, k in launches)
        want[f"cluster {key}: THREADS*MAXV4 + 1 -> wpc=2"] = any(k == key and g[1] == 2 and S // 4 == THREADS * m + 1
                                                                 for (_, _, S), g, k in launches)
        want[f"cluster {key}: more tickets than resident workgroups, ragged then full slices"] = any(
            k == key and B * GROUPS * g[2] > g[3] and g[1] > 1 and (S // 4) % g[1] for (B, _, S), g, k in launches)
        for cpg in (1, 2, 4, 8):
            want[f"cluster {key}: wpc>1 ragged, cpg={cpg}"] = any(k == key and g[0] == cpg and g[1] > 1 and (S // 4) % g[1]
                                                                  for (_, _, S), g, k in launches)
    both = lambda gs: all(g == TWO_STAGE for g in gs.values())                          # noqa: E731
    for r in (1, 2, 3):
        want[f"two-stage by shape: S % 4 = {r}"] = any(S % 4 == r and both(gs) for (_, _, S), gs in G.values())
    want["two-stage by shape: cpg = 10"] = any(C_ == 320 and S % 4 == 0 and both(gs) for (_, C_, S), gs in G.values())
    want["two-stage by shape: wpc * cpg > 128, both directions"] = any(
        S % 4 == 0 and C_ // GROUPS <= FUSED_MAX_CPG and both(gs)
        and -(-S // 4 // (THREADS * FWD_MAXV4)) * (C_ // GROUPS) > FUSED_MAX_CL_RUN for (_, C_, S), gs in G.values())
    want["mixed band: forward cluster, backward two-stage (B=1, C=32)"] = any(
        B == 1 and C_ == 32 and fused(gs["fwd"]) and fused(gs["fwds"]) and gs["bwd"] == TWO_STAGE for (B, C_, S), gs in G.values())
    for S0 in CHUNK_S:
        want[f"two-stage chunking: cpg=2, S={S0}"] = any(C_ == 64 and S == S0 for (_, C_, S), _ in G.values())
    want["two-stage chunking: S % 4 != 0 above two chunks, cpg=2"] = any(
        C_ == 64 and S % 4 and chunks_of(S) > 2 and chunks_of(2 * S) != chunks_of(S) for (_, C_, S), _ in G.values())
    for n in PIVOT_N:
        want[f"pivot: n={n}"] = any(C_ == 32 and S == n for (_, C_, S), _ in G.values())
    for k, s in PRODUCTION.items():
        want[f"production {k}"] = CASES.get(k) == s
    want["production: the 3-D volume of the step stays on the cluster kernels"] = all(fused(g) for g in G["prod_3d_32"][1].values())
    return sorted(k for k, ok in want.items() if not ok)


# ---- fixtures and helpers ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def cluster_mode(ecm, mode):
    """ecm_gn3d_cluster_mode(mode) for the block; afterwards the previous mode is back and a starved cluster (a bounded wait that
    expired: RuntimeError "... timed out") fails THIS test instead of travelling into the next."""
    old = ecm.ops.gn_cluster_mode(mode)
    try:
        yield
    finally:
        ecm.ops.gn_cluster_mode(old)
        ecm.ops.check_async_errors()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _data(shape, skip, seed, dtype=torch.float32):
    """x = 1.7 * randn + 0.3, gamma = 1 + 0.2 * randn, beta = 0.2 * randn, skip = randn, gy = randn (test_hip_parity's recipe)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)                         # noqa: E731
    Cc = shape[1]
    x = (r(*shape) * 1.7 + 0.3).to(dtype)
    gm, bt = 1 + 0.2 * r(Cc), 0.2 * r(Cc)
    sk = r(*shape).to(dtype) if skip else None
    return x, gm, bt, sk, r(*shape)


def _reference(x, gm, bt, sk, relu, gy, dtype, device):
    """The expression in `dtype` on `device` -> (quantities, gy as used).  In fp64 (the reference proper) the tie rule is applied
    to gy; the fp32 draws are given that gy."""
    B, Cc, S = _bcs(x.shape)
    cv = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype, copy=True)      # noqa: E731
    xs = [None if t is None else cv(t).requires_grad_() for t in (x, gm, bt, sk)]
    with torch.no_grad():
        _, mean, rstd = torch.native_group_norm(xs[0].detach(), xs[1].detach(), xs[2].detach(), B, Cc, S, GROUPS, EPS)
    p = F.group_norm(xs[0], GROUPS, xs[1], xs[2], EPS)
    if sk is not None:
        p = p + xs[3]
    y = F.relu(p) if relu else p
    if dtype == torch.float64 and relu:
        tie = p.detach().abs() < TIE
        share = float(tie.float().mean())
        assert share <= TIE_SHARE, f"{share:.2e} of the pre-activations lie within {TIE} of 0: above the cap of {TIE_SHARE}"
        gy = gy.masked_fill(tie.to(gy.device), 0.0)
        del tie
    y.backward(cv(gy))
    q = {"y": y.detach(), "gx": xs[0].grad, "ggamma": xs[1].grad, "gbeta": xs[2].grad, "mean": mean.reshape(B, GROUPS),
         "rstd": rstd.reshape(B, GROUPS)}
    if sk is not None:
        q["gskip"] = xs[3].grad
    return q, gy


def _hip(ecm, x, gm, bt, sk, relu, gy, head=0, g_head=None):
    """ops.group_norm_act forward + backward on fresh copies of the operands -> the same quantities."""
    xs = [None if t is None else t.clone().requires_grad_() for t in (x, gm, bt, sk)]
    out = ecm.ops.group_norm_act(xs[0], xs[1], xs[2], xs[3], relu, head=head)
    y, xh = out if head else (out, None)
    stats = y.grad_fn.saved_tensors[1].clone()                  # (mean, rstd) as the forward kernel wrote them
    if g_head is not None:
        torch.autograd.backward([y, xh], [gy.clone(), g_head.clone()])
    else:
        y.backward(gy.clone())
    q = {"y": y.detach(), "gx": xs[0].grad, "ggamma": xs[1].grad, "gbeta": xs[2].grad, "mean": stats[..., 0], "rstd": stats[..., 1]}
    if sk is not None:
        q["gskip"] = xs[3].grad
    if head:
        q["x_head"] = xh.detach()
    return q


def _units(q64, draws):
    """e32 per quantity: the larger distance of the fp32 draws from fp64."""
    e32 = {}
    for k, ref in q64.items():
        e32[k] = max(float((d[k].to(ref.device).double() - ref).abs().max()) for d in draws)
    return e32


def _compare(label, paths, hip, q64, e32, fails):
    """Section-1 rule for every quantity; prints the ratios, collects the failures (asserted by the caller after all prints)."""
    for k, ref in q64.items():
        if k == "gskip":
            if not torch.equal(hip[k], ref.float()):
                fails.append(f"{label}: gskip differs from the masked gy in {int((hip[k] != ref.float()).sum())} elements")
            continue
        err = float((hip[k].double() - ref).abs().max())
        bound = K * e32[k] + FLOOR * float(ref.abs().max())
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"GNRATIO {paths[k]} {k} {ratio:.3f}   # {label}: err {err:.3e}, e32 {e32[k]:.3e}, max|ref| {float(ref.abs().max()):.3e}")
        if not err <= bound:                                     # (a NaN fails)
            fails.append(f"{label}: {k}: |hip - fp64| = {err:.3e} > {K} * {e32[k]:.3e} + {FLOOR} * {float(ref.abs().max()):.3e}"
                         f" (ratio {ratio:.2f})")


def _path_names(shape, skip, mode, cus):
    g = geoms(shape, cus)
    f = TWO_STAGE if mode == 0 or g["fwds" if skip else "fwd"] == TWO_STAGE else "cluster"
    b = TWO_STAGE if mode == 0 or g["bwd"] == TWO_STAGE else "cluster"
    bl = "bwd:" + b + ("(cluster-stats)" if (f, b) == ("cluster", TWO_STAGE) else "")
    return {"y": "fwd:" + f, "mean": "fwd:" + f, "rstd": "fwd:" + f, "gx": bl, "ggamma": bl, "gbeta": bl}


def _run_case(ecm, cus, name, relu, skip, modes):
    shape = CASES[name]
    x, gm, bt, sk, gy = _data(shape, skip, _seed(name, relu, skip))
    big = x.numel() * 4 * 4 >= BIG_BYTES
    fails, keep = [], []
    try:
        q64, gy = _reference(x, gm, bt, sk, relu, gy, torch.float64, "cuda")
        runs = {}
        for mode in modes:                                       # the kernels first: nothing of this case in fp32 has been freed yet
            with cluster_mode(ecm, mode):
                runs[mode] = [_hip(ecm, x, gm, bt, sk, relu, gy) for _ in range(2)]
            keep.append(runs[mode])
        draws = [_reference(x, gm, bt, sk, relu, gy, torch.float32, "cuda")[0]]
        if not big:
            draws.append(_reference(x, gm, bt, sk, relu, gy, torch.float32, "cpu")[0])
        e32 = _units(q64, draws)
        for mode in modes:
            a, b = runs[mode]
            label = f"{name} relu={int(relu)} skip={int(skip)} mode={mode}"
            _compare(label, _path_names(shape, skip, mode, cus), a, q64, e32, fails)
            for k in a:
                if not torch.equal(a[k], b[k]):
                    fails.append(f"{label}: {k} differs between two runs in {int((a[k] != b[k]).sum())} elements")
        assert not fails, "\n".join(fails)
    finally:
        del keep
        if big:
            torch.cuda.empty_cache()


# ---- 2. path coverage ----------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_class_on_this_device(cus):
    """With this device's CU count (resident workgroups = CUs x 2) every class still has its case -- a failure, not a skip."""
    assert missing_classes(cus) == []


@pytest.mark.parametrize("relu,skip", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_groupnorm_fp64_small(ecm, cus, name, relu, skip):
    """Forward relu x skip, backward (mask, gskip) = (0,0), (2,0), (1,1), with the cluster kernels allowed and switched off."""
    _run_case(ecm, cus, name, relu, skip, (1, 0))


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", sorted(MIXED))
def test_groupnorm_fp64_mixed_band(ecm, cus, name, skip):
    """128 * 5120 < S/4 <= 128 * 8192 at one channel per group: gn_fused_fwd writes the statistics, gn_bwd_partial reads them."""
    _run_case(ecm, cus, name, True, skip, (1, 0))


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("name", sorted(PRODUCTION))
def test_groupnorm_fp64_production(ecm, cus, name, skip):
    _run_case(ecm, cus, name, True, skip, (1,))


# ---- 3. the instantiations only the C ABI reaches -------------------------------------------------------------------------------
def _abi(ecm, keep, x, gm, bt, sk, relu, gy, use_y, want_gskip):
    """ecm_gn3d_fwd + ecm_gn3d_bwd (keep None: exchange memory preset per launch) or _fwd_p + _bwd_p (kept) into NaN-filled outputs."""
    lib, p = ecm.ops._lib, ecm.ops._p
    B, Cc, S = _bcs(x.shape)
    nb = lib.query("ecm_gn3d_scratch_bytes", B, Cc, C.c_longlong(S))
    scratch = torch.empty(nb // 4 + 16, device="cuda")
    nan = lambda t: torch.full_like(t, float("nan"))                                    # noqa: E731
    y, gx, gg, gb, stats = nan(x), nan(x), nan(gm), nan(gm), torch.full((B, GROUPS, 2), float("nan"), device="cuda")
    gskip = nan(x) if want_gskip else None
    dims = (B, Cc, C.c_longlong(S), int(relu))
    kept = () if keep is None else (p(keep), C.c_longlong(keep.numel()))
    sfx = "" if keep is None else "_p"
    lib.call("ecm_gn3d_fwd" + sfx, p(x), p(gm), p(bt), p(sk), p(y), p(stats), p(scratch), C.c_longlong(nb), *kept, *dims,
             C.c_float(EPS), ecm.ops._stream())
    lib.call("ecm_gn3d_bwd" + sfx, p(x), p(stats), p(gm), p(bt), p(y if use_y else None), p(gy), p(gx), p(gskip), p(gg), p(gb),
             p(scratch), C.c_longlong(nb), *kept, *dims, ecm.ops._stream())
    torch.cuda.synchronize()
    q = {"y": y, "gx": gx, "ggamma": gg, "gbeta": gb, "mean": stats[..., 0], "rstd": stats[..., 1]}
    if want_gskip:
        q["gskip"] = gskip
    return q


# (relu, mask from y, gskip written) -> gn_fused_bwd / gn_bwd_partial <0,1>, <1,0>, <2,1>; the forward adds a skip where y is the mask
ABI_COMBOS = {"norelu_gskip": (False, False, True), "mask_y_no_gskip": (True, True, False), "mask_x_gskip": (True, False, True)}
ABI_SHAPES = {"cluster": (2, 64, 4 * _P), "two_stage": (1, 320, 40000)}


@pytest.mark.parametrize("combo", sorted(ABI_COMBOS))
@pytest.mark.parametrize("kind", sorted(ABI_SHAPES))
def test_groupnorm_abi_only_instantiations(ecm, cus, kind, combo):
    """The three (mask, gskip) pairs ops.GroupNormAct never produces, through ecm_gn3d_bwd and ecm_gn3d_bwd_p: against fp64 like
    every other path; stateless and kept-exchange-memory entry points bit-identical; the kept memory back in its preset state."""
    relu, use_y, want_gskip = ABI_COMBOS[combo]
    shape = ABI_SHAPES[kind]
    assert (geoms(shape, cus)["bwd"] != TWO_STAGE) == (kind == "cluster") and (geoms(shape, cus)["fwds"] != TWO_STAGE) == (kind == "cluster")
    skip = use_y
    x, gm, bt, sk, gy = _data(shape, skip, _seed("abi", kind, combo))
    q64, gy = _reference(x, gm, bt, sk, relu, gy, torch.float64, "cuda")
    if want_gskip:                                               # the masked gradient, whether or not a residual operand exists
        q64["gskip"] = gy.double() * (q64["y"] > 0) if relu else gy.double()
    else:
        q64.pop("gskip", None)
    lib = ecm.ops._lib
    keep = torch.empty(lib.query("ecm_gn3d_cluster_bytes", shape[0]), dtype=torch.uint8, device="cuda")
    lib.call("ecm_gn3d_cluster_preset", ecm.ops._p(keep), C.c_longlong(keep.numel()), ecm.ops._stream())
    fails = []
    with cluster_mode(ecm, 1):
        a = _abi(ecm, None, x, gm, bt, sk, relu, gy, use_y, want_gskip)
        b = _abi(ecm, keep, x, gm, bt, sk, relu, gy, use_y, want_gskip)
        b2 = _abi(ecm, keep, x, gm, bt, sk, relu, gy, use_y, want_gskip)          # on the memory the first pair handed back
    draws = [_reference(x, gm, bt, sk, relu, gy, torch.float32, d)[0] for d in ("cuda", "cpu")]
    e32 = _units({k: v for k, v in q64.items() if k != "gskip"}, draws)
    label = f"abi {kind} {combo}"
    paths = {k: ("abi:" + v) for k, v in _path_names(shape, skip, 1, cus).items()}
    _compare(label, paths, a, q64, e32, fails)
    for k in a:
        for other, what in ((b, "ecm_gn3d_*_p"), (b2, "a second ecm_gn3d_*_p call")):
            if not torch.equal(a[k], other[k]):
                fails.append(f"{label}: {k}: {what} differs from the stateless entry points in {int((a[k] != other[k]).sum())} elements")
    if not bool((keep == 0xFF).all()):
        fails.append(f"{label}: {int((keep != 0xFF).sum())} bytes of the kept exchange memory are not back at 0xFF")
    assert not fails, "\n".join(fails)


# ---- 4. head > 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("kind", sorted(ABI_SHAPES))
def test_groupnorm_head_fork(ecm, cus, kind, with_grad):
    """group_norm_act(head=h) also returns x[:h] and adds that consumer's gradient into gx[:h]: y and gx bit-identical to the
    head = 0 call plus an explicit add -- also when the second output receives no gradient at all."""
    shape = {"cluster": (3, 64, 4 * _P), "two_stage": (3, 320, 10000)}[kind]
    assert (geoms(shape, cus)["bwd"] != TWO_STAGE) == (kind == "cluster")
    h = 2
    x, gm, bt, sk, gy = _data(shape, True, _seed("head", kind))
    g_head = torch.randn(h, *shape[1:], device="cuda", generator=torch.Generator(device="cuda").manual_seed(_seed("gh", kind)))
    with cluster_mode(ecm, 1):
        base = _hip(ecm, x, gm, bt, sk, True, gy)
        fork = _hip(ecm, x, gm, bt, sk, True, gy, head=h, g_head=g_head if with_grad else None)
    assert torch.equal(fork["x_head"], x[:h])
    want_gx = base["gx"].clone()
    if with_grad:
        want_gx[:h] += g_head
    for k in base:
        assert torch.equal(fork[k], want_gx if k == "gx" else base[k]), (kind, with_grad, k)


# ---- 5. bf16 storage, every remainder --------------------------------------------------------------------------------------------
BF = torch.bfloat16
# S % 8 = 0..7 at one and two channels per group ((cpg * S) % 8 == 0 with S % 8 == 4 at C = 64: vector statistics, scalar apply),
# eight channels per group with an odd S (the same split at S % 8 odd), and two sizes above one chunk
BF16_SHAPES = ([(2, 32, 1000 + r) for r in range(8)] + [(1, 64, 1000 + r) for r in range(8)] +
               [(1, 256, 1001), (1, 256, 1007), (1, 32, 40000), (1, 32, 40003), (1, 64, 40003)])


def _want32(x, gm, bt, sk, relu):
    w = F.group_norm(x.float(), GROUPS, gm, bt, EPS)
    if sk is not None:
        w = w + sk.float()
    return w.clamp_min(0) if relu else w


@pytest.mark.parametrize("relu,skip", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("shape", BF16_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_bf16_remainders(ecm, shape, relu, skip):
    """bf16 outputs within 1 bf16 ulp of fp32 F.group_norm of the same bf16 operands (test_hip_bf16_infer's yardstick); the fp32
    outputs of the bf16 -> fp32 form and the statistics of a bf16 tensor by the fp64 rule of this module; the dual store's bf16
    copy is the fp32 result rounded to bf16, bit for bit."""
    from test_hip_bf16_infer import _within_ulp
    B, Cc, S = _bcs(shape)
    x32, gm, bt, sk, _ = _data(shape, skip, _seed("bf16", shape, relu, skip))
    x16 = x32.to(BF)
    sk = None if sk is None else sk.to(BF)
    fails = []
    label = f"bf16 {shape} relu={int(relu)} skip={int(skip)}"
    with torch.no_grad():
        y_bb = ecm.ops.group_norm_act(x16, gm, bt, sk, relu, out_dtype=BF)
        y_fb = ecm.ops.group_norm_act(x32, gm, bt, sk, relu, out_dtype=BF)
        y_f = ecm.ops.group_norm_act_bf16_f32(x16, gm, bt, sk, relu, dual=False)
        y_d32, y_d16 = ecm.ops.group_norm_act_bf16_f32(x16, gm, bt, sk, relu, dual=True)
        stats = ecm.ops._gn_stats(x16)
        ecm.ops.check_async_errors()
        assert y_bb.dtype == BF and y_fb.dtype == BF and y_d16.dtype == BF and y_f.dtype == torch.float32 == y_d32.dtype
        _within_ulp(y_bb, _want32(x16, gm, bt, sk, relu), label + " bf16 -> bf16")
        _within_ulp(y_fb, _want32(x32, gm, bt, sk, relu), label + " fp32 -> bf16")
        assert torch.equal(y_d32, y_f), label + ": the dual store's fp32 result differs from the single store's"
        assert torch.equal(y_d16.view(torch.int16), y_d32.to(BF).view(torch.int16)), label + ": bf16 copy != fp32 result rounded to bf16"
        # fp32 result and statistics: fp64 of the same bf16 values, unit = torch's fp32 on the device and on the CPU
        q64, draws = {}, [{}, {}]
        for q, dtype, dev in [(q64, torch.float64, "cuda"), (draws[0], torch.float32, "cuda"), (draws[1], torch.float32, "cpu")]:
            cv = lambda t: None if t is None else t.to(device=dev, dtype=dtype)         # noqa: E731
            w = F.group_norm(cv(x16), GROUPS, cv(gm), cv(bt), EPS)
            if sk is not None:
                w = w + cv(sk)
            q["y"] = w.clamp_min(0) if relu else w
            _, mean, rstd = torch.native_group_norm(cv(x16), cv(gm), cv(bt), B, Cc, S, GROUPS, EPS)
            q["mean"], q["rstd"] = mean.reshape(B, GROUPS), rstd.reshape(B, GROUPS)
        e32 = _units(q64, draws)
        hip = {"y": y_f, "mean": stats[..., 0], "rstd": stats[..., 1]}
        _compare(label, {"y": "bf16->fp32:apply", "mean": "bf16:stats", "rstd": "bf16:stats"}, hip, q64, e32, fails)
    assert not fails, "\n".join(fails)
