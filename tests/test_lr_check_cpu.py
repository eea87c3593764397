"""The left-right consistency check, the part that needs no GPU: `lr_check_t` below, a torch restatement
of the definitions at any dtype and on any device -- the reference of tests/test_hip_lr_check.py -- checked in fp64 against
closed forms; the ABI additions; the refusals of ops.lr_check and cross_check that come before any device work; and the
borderline share of the GPU test's random cases (pixels whose kind differs between the fp32 and the fp64 restatement).

Definitions, per pixel with d = dl[b,y,x]:  xr = x - d, x0 = floor(xr), x1 = min(x0 + 1, W-1), t = xr - x0,
r = dr[x0] + t (dr[x1] - dr[x0]), tol = max(threshold, rel d), error = |d - r|;  kind 3 where d is not finite or xr leaves
[0, W-1] (error +inf), else 0 where error <= tol, else 1 where r is finite and r > d, else 2 (error +inf for a non-finite r).
filled = d where kind is 0, else dl at the nearest kind-0 column on the left or on the right, the one with the smaller
disparity (the left on a tie, the only one if the other does not exist), 0 and src = -1 if the row has none."""
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

NEW_ENTRIES = ("ecm_lr_check_fwd", "ecm_lr_check_max_width")
INF = float("inf")
# the random cases of the GPU test: (name, seed, shape)
FLOAT_CASES = [("2x5x200", 1701, (2, 5, 200)), ("1x3x1248", 1702, (1, 3, 1248))]
BORDERLINE_CAP = 1e-3


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def fill_t(dl, cons):
    """(filled, src) of a row-wise fill of dl [B,H,W] from the columns where `cons` holds."""
    W = dl.shape[-1]
    idx = torch.arange(W, device=dl.device).expand(dl.shape)
    Lx = torch.where(cons, idx, torch.full_like(idx, -1)).cummax(2).values
    Rx = torch.where(cons, idx, torch.full_like(idx, W)).flip(2).cummin(2).values.flip(2)
    hl, hr = Lx >= 0, Rx < W
    a, b = dl.gather(2, Lx.clamp(min=0)), dl.gather(2, Rx.clamp(max=W - 1))
    right = hr & (~hl | (b < a))
    src = torch.where(cons, idx, torch.where(right, Rx, Lx))          # Lx is -1 where neither exists
    filled = torch.where(src >= 0, dl.gather(2, src.clamp(min=0)), torch.zeros_like(dl))
    return filled, src


def lr_check_t(dl, dr, threshold, rel, mirrored):
    """(error, kind, filled, src) of dl, dr [B,H,W] in their own dtype; kind in that dtype, src int64."""
    W = dl.shape[-1]
    if mirrored:
        dr = dr.flip(2)
    x = torch.arange(W, device=dl.device, dtype=dl.dtype).expand(dl.shape)
    xr = x - dl
    oov = ~torch.isfinite(dl) | (xr < 0) | (xr > W - 1)
    xs = torch.where(oov, torch.zeros_like(xr), xr)
    f = xs.floor()
    x0 = f.long()
    r0, r1 = dr.gather(2, x0), dr.gather(2, (x0 + 1).clamp(max=W - 1))
    r = r0 + (xs - f) * (r1 - r0)
    rfin = torch.isfinite(r)
    inf = torch.full_like(dl, INF)
    error = torch.where(oov | ~rfin, inf, (dl - r).abs())
    tol = torch.maximum(torch.full_like(dl, threshold), rel * dl)
    cons = ~oov & (error <= tol)
    one = torch.ones_like(dl)
    kind = torch.where(oov, 3 * one, torch.where(cons, 0 * one, torch.where(rfin & (r > dl), one, 2 * one)))
    filled, src = fill_t(dl, cons)
    return error, kind, filled, src


def float_case(seed, shape):
    """A random case of the GPU test, fp32 on the CPU: every row of dl is a ramp a + g x inside [0, 40) with seeded random a
    and g, dr the right view that is consistent with it -- left x is right x' = (1 - g) x - a, so dr(x') = a + g (x' + a) /
    (1 - g), linear in x': the interpolation reproduces it -- plus seeded uniform noise of up to 4 px on every pixel."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    a = 30 * torch.rand(B, H, 1, generator=gen, dtype=torch.float64)
    g = (torch.rand(B, H, 1, generator=gen, dtype=torch.float64) * 2 - 1) * 9.9 / W
    a = a.clamp(min=-(g * (W - 1)).clamp(max=0))                       # the ramp stays >= 0 (and < 40: 30 + 9.9)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    dl = a + g * x
    dr = a + g * (x + a) / (1 - g) + (torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 8 - 4)
    return dl.float(), dr.float()


def kernel_constants():
    """The constexpr ints of csrc/lr_check.hip by name (the GPU test places its runs at the boundaries they define)."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "lr_check.hip")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr) and "INT_MAX" not in expr:
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


def run64(dl, dr, threshold=1.0, rel=0.0, mirrored=False):
    return lr_check_t(torch.as_tensor(dl, dtype=torch.float64), torch.as_tensor(dr, dtype=torch.float64), threshold, rel, mirrored)


# ---- closed forms, fp64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 7])
def test_constant_plane(k):
    B, H, W = 2, 3, 20
    d = torch.full((B, H, W), float(k), dtype=torch.float64)
    error, kind, filled, src = run64(d, d)
    x = torch.arange(W).expand(B, H, W)
    assert torch.equal(kind, torch.where(x < k, 3.0, 0.0).double())
    assert bool((error[x >= k] == 0).all()) and bool(torch.isinf(error[x < k]).all())
    assert torch.equal(src, torch.where(x < k, k, x)) and torch.equal(filled, d)      # the border takes column k's value


def box_scene(H=8, W=40, b=2.0, f=6.0, x_lo=20, x_hi=30, y_lo=2, y_hi=6):
    """A fronto-parallel box (disparity f, left-view columns [x_lo, x_hi), rows [y_lo, y_hi)) before a background (b), both
    views written down from the geometry: a left pixel x at disparity d is right pixel x - d."""
    dl, dr = torch.full((1, H, W), b, dtype=torch.float64), torch.full((1, H, W), b, dtype=torch.float64)
    dl[0, y_lo:y_hi, x_lo:x_hi] = f
    dr[0, y_lo:y_hi, x_lo - int(f):x_hi - int(f)] = f
    return dl, dr


def test_foreground_box():
    b, f, x_lo, x_hi, y_lo, y_hi = 2.0, 6.0, 20, 30, 2, 6
    dl, dr = box_scene()
    error, kind, filled, src = run64(dl, dr)
    want = torch.zeros_like(dl)
    want[..., :int(b)] = 3                                             # the left image border
    want[0, y_lo:y_hi, x_lo - int(f - b):x_lo] = 1                     # background that the box hides from the right camera
    assert torch.equal(kind, want)
    strip = kind == 1
    assert bool((error[strip] == f - b).all()) and bool((filled[strip] == b).all())
    assert bool((src[0, y_lo:y_hi, x_lo - int(f - b):x_lo] == x_lo - int(f - b) - 1).all())    # from the left: the background
    assert torch.equal(filled, torch.where(strip, torch.full_like(dl, b), dl))


def test_mirrored_is_the_flipped_right_plane():
    dl, dr = (t.double() for t in float_case(3, (2, 3, 50)))
    plain = run64(dl, dr, 1.0, 0.05, False)
    flipped = run64(dl, dr.flip(2), 1.0, 0.05, True)
    assert all(torch.equal(a, b) for a, b in zip(plain, flipped))
    assert not torch.equal(plain[1], run64(dl, dr.flip(2), 1.0, 0.05, False)[1])


def test_threshold_is_inclusive_and_rel_takes_over():
    W = 40
    dl, dr = torch.full((1, 1, W), 4.0, dtype=torch.float64), torch.full((1, 1, W), 4.0, dtype=torch.float64)
    dl[0, 0, 10], dl[0, 0, 11], dl[0, 0, 12] = 4.5, 4.625, 3.5          # errors 0.5, 0.625, 0.5 against r = 4
    error, kind, _, _ = run64(dl, dr, threshold=0.5)
    assert error[0, 0, 10] == 0.5 and kind[0, 0, 10] == 0 and kind[0, 0, 12] == 0
    assert error[0, 0, 11] == 0.625 and kind[0, 0, 11] == 2            # r < d: a mismatch
    dl = torch.full((1, 1, W), 20.0, dtype=torch.float64)
    dr = torch.full((1, 1, W), 20.75, dtype=torch.float64)
    assert bool((run64(dl, dr, 0.5, 0.0)[1][0, 0, 20:] == 1).all())    # 0.75 > 0.5, r > d: occluded
    assert bool((run64(dl, dr, 0.5, 0.05)[1][0, 0, 20:] == 0).all())   # rel d = 1.0 takes over
    assert bool((run64(dl, dr, 0.5, 0.03)[1][0, 0, 20:] == 1).all())   # rel d = 0.6 does not reach


@pytest.mark.parametrize("bad", [float("nan"), INF, -INF])
def test_non_finite_inputs(bad):
    W = 16
    base = torch.full((1, 2, W), 2.0, dtype=torch.float64)
    dl = base.clone()
    dl[0, 0, 9] = bad
    error, kind, filled, src = run64(dl, base)
    assert kind[0, 0, 9] == 3 and error[0, 0, 9] == INF and filled[0, 0, 9] == 2 and src[0, 0, 9] == 8
    others = torch.arange(W) != 9
    assert torch.equal(kind[0, 0, others], kind[0, 1, others]) and kind[0, 1, 9] == 0      # nothing else changes
    dr = base.clone()
    dr[0, 0, 5] = bad                    # d = 2: column 7 reads it as dr[x0]; column 6 as dr[x1] at t = 0, and 0 * inf is NaN
    error, kind, _, _ = run64(base, dr)
    assert kind[0, 0, 7] == 2 and error[0, 0, 7] == INF and kind[0, 0, 6] == 2 and error[0, 0, 6] == INF
    assert kind[0, 0, 8] == 0 and kind[0, 0, 5] == 0 and bool((kind[0, 1, 2:] == 0).all())


def test_row_without_a_consistent_pixel():
    dl, dr = torch.full((1, 2, 12), 1.0, dtype=torch.float64), torch.full((1, 2, 12), 1.0, dtype=torch.float64)
    dr[0, 0] = 5.0
    _, kind, filled, src = run64(dl, dr)
    assert bool((kind[0, 0, 1:] == 1).all()) and bool((filled[0, 0] == 0).all()) and bool((src[0, 0] == -1).all())
    assert bool((filled[0, 1] == 1).all())


def test_fill_takes_the_background_and_the_left_on_a_tie():
    dl = torch.tensor([[[0.0, 5.0, 9.0, 9.0, 2.0, 9.0, 2.0, 9.0]]], dtype=torch.float64)
    cons = torch.tensor([[[False, True, False, False, True, False, True, False]]])
    filled, src = fill_t(dl, cons)
    assert src.tolist() == [[[1, 1, 4, 4, 4, 4, 6, 6]]]                # column 5: 2 == 2, the left one
    assert filled.tolist() == [[[5.0, 5.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]]]


# ---- the random cases of the GPU test: how many pixels fp32 itself cannot classify ------------------------------------------------------
@pytest.mark.parametrize("name,seed,shape", FLOAT_CASES, ids=[c[0] for c in FLOAT_CASES])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("threshold,rel", [(1.0, 0.0), (0.5, 0.05)])
def test_borderline_share_of_the_float_cases(name, seed, shape, mirrored, threshold, rel):
    dl, dr = float_case(seed, shape)
    assert float(dl.min()) >= 0 and float(dl.max()) < 40
    if mirrored:
        dr = dr.flip(2).contiguous()
    k32 = lr_check_t(dl, dr, threshold, rel, mirrored)[1]
    k64 = lr_check_t(dl.double(), dr.double(), threshold, rel, mirrored)[1]
    share = float((k32.double() != k64).double().mean())
    kinds = [float((k64 == k).double().mean()) for k in range(4)]
    print(f"LRBORDER {name} {share:.5f}   # kinds 0..3: {kinds}")
    assert share <= BORDERLINE_CAP
    assert min(kinds[:3]) > 0.02 and kinds[3] > 0                      # every class is there to be got wrong


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_mod():
    import ecm_amd
    if not os.path.exists(ecm_amd._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm_amd._lib


def test_header_and_prototypes_hold_the_new_entries(lib_mod):
    for name in NEW_ENTRIES:
        assert name in declared() and name in lib_mod.PROTOTYPES, name
    assert lib_mod.missing_symbols() == []
    assert lib_mod.query("ecm_abi_version") >= 10
    assert len(lib_mod.PROTOTYPES["ecm_lr_check_fwd"][1]) == 11


def test_max_width_needs_no_gpu(lib_mod):
    import ecm_amd
    assert lib_mod.query("ecm_lr_check_max_width") >= 4096
    assert ecm_amd.ops.lr_check_max_width() == lib_mod.query("ecm_lr_check_max_width") == kernel_constants()["MAX_W"]
    k = kernel_constants()
    assert k["SWEEP"] == k["THREADS"] * k["CHUNK"] and k["MAX_W"] % k["SWEEP"] == 0 and k["WAVE"] == 64


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    lib = lib_mod.load()
    assert lib.ecm_lr_check_fwd(None, None, None, None, 1, 1, 1, 1.0, 0.0, 0, None) == -1
    import ctypes as C
    p = C.c_void_p(64)                                                 # never dereferenced: every call below returns first
    assert lib.ecm_lr_check_fwd(p, p, p, None, 1, 1, 0, 1.0, 0.0, 0, None) == -1
    assert lib.ecm_lr_check_fwd(p, p, p, None, 1, 1, 8, -1.0, 0.0, 0, None) == -1
    assert lib.ecm_lr_check_fwd(p, p, p, None, 1, 1, 8, 1.0, float("nan"), 0, None) == -1
    assert lib.ecm_lr_check_fwd(p, p, p, None, 1, 1, 8, INF, 0.0, 0, None) == -1
    wide = lib_mod.query("ecm_lr_check_max_width") + 1
    assert lib.ecm_lr_check_fwd(p, p, p, None, 1, 1, wide, 1.0, 0.0, 0, None) == -2
    assert lib.ecm_lr_check_fwd(p, p, p, None, 1 << 16, 1 << 15, 8, 1.0, 0.0, 0, None) == -2     # B * H = 2^31 rows


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
def test_op_refusals():
    import ecm_amd
    ops = ecm_amd.ops
    d = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.lr_check(d, d)
    for kw in ({"threshold": -1.0}, {"threshold": float("nan")}, {"threshold": INF}, {"rel": -0.1}, {"rel": float("nan")},
               {"threshold": "1"}, {"rel": None}, {"threshold": True}):
        with pytest.raises(ValueError, match="lr_check"):
            ops.lr_check(d, d, **kw)
    assert ops.check_lr_tolerances(1, 0) == (1.0, 0.0)
    sig = inspect.signature(ops.lr_check)
    assert list(sig.parameters) == ["disp_l", "disp_r", "threshold", "rel", "mirrored", "with_source"]
    assert [sig.parameters[n].default for n in ("threshold", "rel", "mirrored", "with_source")] == [1.0, 0.0, False, False]


def test_cross_check_is_wired_and_refuses_on_the_cpu():
    import ecm_amd
    from ecm_amd import models
    assert models.CrossCheck._fields == ("disparity", "disparity_right", "error", "kind", "filled")
    sig = inspect.signature(models._ECMNet.cross_check)
    assert list(sig.parameters) == ["self", "left", "right", "threshold", "rel", "head"] and sig.parameters["head"].default == 2
    x = torch.zeros(1, 3, 64, 128)
    for name in ("cmfsm", "cmf", "cmfsm_sub_8"):
        net = ecm_amd.get_model(name)
        for bad in (-1, 3, 1.0, True, None):
            with pytest.raises(ValueError, match="head"):
                net.cross_check(x, x, head=bad)
        with pytest.raises(ValueError, match="threshold"):
            net.cross_check(x, x, threshold=-1.0)
        with pytest.raises(ValueError, match="rel"):
            net.cross_check(x, x, rel=float("inf"))
    assert all(hasattr(cls, "cross_check") for cls in models._MODELS.values())
