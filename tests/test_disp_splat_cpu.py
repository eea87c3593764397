"""The disparity splat, the part that needs no GPU: `splat_t` below, a torch fp32 restatement of the
definition -- the reference of tests/test_hip_disp_splat.py, which compares bit for bit -- checked against closed forms, the
invariants it gives ops.lr_check, ties and special values; then the ABI additions and the refusals of ops.disparity_splat, of
self_check and of models.occlusion_check that come before any device work.

Definition, per row of d [B,H,W] fp32: pixel x is a candidate iff d is finite and xr = (float)x - d (one fp32 subtraction) lies in
[0, W-1]; with f = floor(xr) it lands on x0 = f and, if xr > f, on x1 = min(x0 + 1, W-1).  Per right column the candidate with
the largest key wins: the order-preserving image of the float's bits (all bits flipped if the sign bit is set, else the sign bit
set), then the source column.  right = the winner's d bit for bit, 0.0 for a hole; src = its column, -1 for a hole.

splat_t packs the key as image * 4096 + column in an int64 (W <= 4096 = MAX_W; image < 2^32, so the key is below 2^44) and
reduces with scatter_reduce_("amax"): an integer maximum, as the kernel's."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from test_abi_types import declared
from test_lr_check_cpu import lr_check_t

NEW_ENTRIES = ("ecm_disp_splat_fwd", "ecm_disp_splat_max_width")
NAN, INF = float("nan"), float("inf")
COLS = 4096                                   # the packing of splat_t's key: column < COLS
SIGN = 1 << 31
MASK = (1 << 32) - 1


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def splat_t(d):
    """(right, src) of d [B,H,W] fp32, on d's device: right fp32, src int64."""
    assert d.dtype == torch.float32 and d.dim() == 3 and d.shape[2] <= COLS
    W = d.shape[2]
    col = torch.arange(W, device=d.device).expand(d.shape)
    xr = col.to(torch.float32) - d
    cand = torch.isfinite(d) & (xr >= 0) & (xr <= W - 1)
    f = torch.where(cand, xr, torch.zeros_like(xr)).floor()
    x0 = f.long()
    two = cand & (xr > f)
    x1 = (x0 + 1).clamp(max=W - 1)
    bits = d.contiguous().view(torch.int32).long() & MASK
    image = torch.where(bits >= SIGN, MASK - bits, bits | SIGN)
    key = image * COLS + col
    best = torch.zeros(d.shape, dtype=torch.int64, device=d.device)
    best.scatter_reduce_(2, x0, torch.where(cand, key, torch.zeros_like(key)), "amax")
    best.scatter_reduce_(2, x1, torch.where(two, key, torch.zeros_like(key)), "amax")
    hole = best == 0
    image = best // COLS
    bits = torch.where(image >= SIGN, image - SIGN, MASK - image)
    bits = torch.where(bits >= SIGN, bits - (1 << 32), bits).to(torch.int32)
    right = torch.where(hole, torch.zeros_like(d), bits.view(torch.float32))
    src = torch.where(hole, torch.full_like(best, -1), best % COLS)
    return right, src


def kernel_constants():
    """The constexpr ints of csrc/disp_splat.hip by name."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "disp_splat.hip")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr):
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


# ---- the cases the GPU test shares ------------------------------------------------------------------------------------------------------
def step_case(B=1, H=2):
    """Background 5.25 for 100 columns, foreground 30.5 for 60, background 7.0 for 96: W = 256."""
    row = torch.cat([torch.full((100,), 5.25), torch.full((60,), 30.5), torch.full((96,), 7.0)])
    return row.expand(B, H, 256).contiguous()


def ramp_case(W, slope, B=1, H=2):
    """d = a + slope x, a chosen so that the ramp stays >= 2 px."""
    x = torch.arange(W, dtype=torch.float32)
    a = 2.0 + max(0.0, -slope * (W - 1))
    return (a + slope * x).expand(B, H, W).contiguous()


def check(d, threshold=1.0, rel=0.0):
    """lr_check_t of d against its own splat: (error, kind, filled, src)."""
    return lr_check_t(d, splat_t(d)[0], threshold, rel, False)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 7])
def test_constant_integral_plane(k):
    B, H, W = 2, 3, 20
    right, src = splat_t(torch.full((B, H, W), float(k)))
    x = torch.arange(W).expand(B, H, W)
    landed = x <= W - 1 - k
    assert torch.equal(right, torch.where(landed, float(k), 0.0))
    assert torch.equal(src, torch.where(landed, x + k, -1))


def test_step_hides_the_band_plus_one_column():
    d = step_case()
    error, kind, _, _ = check(d)
    occluded = (kind == 1).sum(2)
    assert occluded.tolist() == [[26, 26]]                               # the 25.25 px band plus the one-column bleed
    assert not bool((kind == 2).any())
    assert bool((kind[0, 0, 74:100] == 1).all())                        # the background just left of the foreground
    # column 74 is the bleed: x - d = 68.75 mixes its own 5.25 on column 68 with the foreground's 30.5 on column 69
    assert float(error[0, 0, 74]) == 0.75 * (30.5 - 5.25) and bool((error[0, 0, 75:100] == 30.5 - 5.25).all())
    right, src = splat_t(d)
    # the foreground (columns 100..159, d = 30.5) lands on 69..129 (two columns each: 69.5 -> 69 and 70)
    assert bool((right[0, 0, 69:130] == 30.5).all()) and src[0, 0, 69] == 100 and src[0, 0, 129] == 159
    # where it uncovers the far background (7.0 lands from 153 on) nothing landed: holes
    assert bool((src[0, 0, 130:153] == -1).all()) and bool((right[0, 0, 130:153] == 0).all()) and src[0, 0, 153] == 160


# ---- invariants -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.3, -0.3])
def test_ramps_stay_consistent(slope):
    d = ramp_case(200, slope)
    error, kind, _, _ = check(d)
    inview = kind != 3
    assert bool((kind[inview] == 0).all()) and int(inview.sum()) > 100
    worst = float(error[inview].max())
    print(f"SPLATRAMP slope {slope}: worst error {worst:.7f} px")
    # 0.36 in exact arithmetic, at slope 0.3: x - d steps by 0.7, and at fraction t = 0.2 the winners of the two columns read lie
    # 1 and 2 sources on, 0.3 * (0.8 * 1 + 0.2 * 2); at slope -0.3 it steps by 1.3 and the worst is 0.18.  In fp32 d < 64 carries half an ulp (2^-19) per value and the interpolation two
    # more roundings of that size: 4 * 2^-18 covers them.
    assert worst <= 0.36 + 4 * 2.0 ** -18


def noise_case(seed, shape, lo, hi):
    gen = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, generator=gen)


@pytest.mark.parametrize("name", ["step", "ramp_up", "ramp_down", "noise", "signed_noise"])
def test_no_mismatch_and_no_negative_error(name):
    d = {"step": step_case(), "ramp_up": ramp_case(200, 0.3), "ramp_down": ramp_case(200, -0.3),
         "noise": noise_case(21, (2, 4, 300), 0.0, 150.0), "signed_noise": noise_case(22, (2, 4, 300), -75.0, 75.0)}[name]
    right, src = splat_t(d)
    error, kind, _, _ = lr_check_t(d, right, 1.0, 0.0, False)
    assert bool(((kind == 0) | (kind == 1) | (kind == 3)).all())
    fin = torch.isfinite(error)
    assert bool((error[fin] >= 0).all()) and torch.equal(fin, kind != 3)
    # every in-view pixel reads columns it wrote to: what stands there is at least its own disparity
    x = torch.arange(d.shape[2]).expand(d.shape)
    xr = x.float() - d
    x0 = xr.floor().long().clamp(0, d.shape[2] - 1)
    assert bool((right.gather(2, x0)[kind != 3] >= d[kind != 3]).all())
    # a winner's value is its source's, bit for bit
    got = src >= 0
    assert torch.equal(right[got].view(torch.int32), d.gather(2, src.clamp(min=0))[got].view(torch.int32))
    assert bool((right[~got].view(torch.int32) == 0).all())


# ---- ties and special values --------------------------------------------------------------------------------------------------------------
def test_the_larger_disparity_wins_and_the_larger_column_wins_a_tie():
    d = torch.tensor([[[2.0, 2.0, 2.0, 1.0, 2.0, 9.0]]])                # x - d = -2, -1, 0, 2, 2, -4
    right, src = splat_t(d)
    assert src[0, 0].tolist() == [2, -1, 4, -1, -1, -1]                  # column 2: d = 2 from column 4 beats d = 1 from column 3
    assert right[0, 0].tolist() == [2.0, 0.0, 2.0, 0.0, 0.0, 0.0]
    d = torch.tensor([[[0.0, 1.0, 1.0, 1.0]]])                           # x - d = 0, 0, 1, 2: column 0 gets d = 0 and d = 1
    right, src = splat_t(d)
    assert src[0, 0].tolist() == [1, 2, 3, -1] and right[0, 0].tolist() == [1.0, 1.0, 1.0, 0.0]
    # equal disparities on one column: 3.5 at 10 (6.5 -> 6, 7) and 3.5 at 11 (7.5 -> 7, 8): column 7 takes source 11
    d = torch.full((1, 1, 16), NAN)
    d[0, 0, 10], d[0, 0, 11] = 3.5, 3.5
    right, src = splat_t(d)
    assert src[0, 0, 6:9].tolist() == [10, 11, 11] and int((src >= 0).sum()) == 3


def image_of(v):
    """The high half of the key of the fp32 value v, as a Python int."""
    bits = torch.tensor([v], dtype=torch.float32).view(torch.int32).long().item() & MASK
    return MASK - bits if bits >= SIGN else bits | SIGN


def test_negative_zero_loses_to_positive_zero():
    d = torch.full((1, 1, 8), NAN)
    d[0, 0, 3] = -0.0
    right, src = splat_t(d)
    assert src[0, 0, 3] == 3 and right[0, 0, 3].view(torch.int32) == -(1 << 31)        # -0.0 lands as itself, bit for bit
    d = torch.tensor([[[NAN, -0.0, 1.0, NAN]]])                          # column 1 gets -0.0 (from 1) and 1.0 (from 2): 1.0 wins
    assert splat_t(d)[1][0, 0].tolist() == [-1, 2, -1, -1]
    # two zeros meet on one column only from one source column (x - 0 = x), so the order of the keys is what decides it
    assert image_of(-1.0) < image_of(-0.0) < image_of(0.0) < image_of(1e-45) < image_of(1.0) < image_of(3.4e38)
    assert image_of(-0.0) == 0x7FFFFFFF and image_of(0.0) == 0x80000000
    assert image_of(-3.4028234663852886e38) == 0x00800000               # the lowest finite float: every key is above 0, the hole


def test_negative_disparities_splat_to_the_right():
    d = torch.full((1, 1, 12), NAN)
    d[0, 0, 2], d[0, 0, 5] = -3.0, -2.5
    right, src = splat_t(d)
    assert src[0, 0].tolist() == [-1] * 5 + [2, -1, 5, 5] + [-1] * 3      # 2 -> 5; 5 -> 7.5 -> 7 and 8
    assert right[0, 0, 5] == -3.0 and right[0, 0, 7] == -2.5 and right[0, 0, 8] == -2.5


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_non_finite_values_never_splat(bad):
    d = torch.full((1, 2, 16), 2.0)
    d[0, 0, ::7] = bad
    right, src = splat_t(d)
    assert bool(torch.isfinite(right).all())
    assert src[0, 1].tolist() == list(range(2, 16)) + [-1, -1]
    want = [c + 2 if (c + 2) % 7 else -1 for c in range(14)] + [-1, -1]
    assert src[0, 0].tolist() == want
    assert bool(torch.isfinite(splat_t(torch.full((1, 1, 5), bad))[0]).all()) and bool((splat_t(torch.full((1, 1, 5), bad))[1] == -1).all())


def test_the_ends_of_the_view_are_in_and_an_integral_landing_writes_one_column():
    W = 10
    d = torch.full((1, 1, W), NAN)
    d[0, 0, 4] = 4.0                                                     # xr = 0 exactly
    right, src = splat_t(d)
    assert src[0, 0].tolist() == [4] + [-1] * (W - 1)
    d = torch.full((1, 1, W), NAN)
    d[0, 0, 6] = -3.0                                                    # xr = W-1 exactly
    right, src = splat_t(d)
    assert src[0, 0].tolist() == [-1] * (W - 1) + [6]
    d = torch.full((1, 1, W), NAN)
    d[0, 0, 6] = -3.000001                                               # 6 - d rounds to the float after 9: out
    assert bool((splat_t(d)[1] == -1).all())
    d[0, 0, 6] = -3.0000002                                              # the float before -3, but 6 - d rounds to 9: the rule is on
    assert splat_t(d)[1][0, 0].tolist() == [-1] * (W - 1) + [6]          # the fp32 difference, so it is in, on one column
    d = torch.full((1, 1, W), NAN)
    d[0, 0, 4] = 4.0000005                                               # just below 0: out
    assert bool((splat_t(d)[1] == -1).all())
    d = torch.full((1, 1, W), NAN)
    d[0, 0, 6] = -2.5                                                    # xr = 8.5: columns 8 and 9
    assert splat_t(d)[1][0, 0].tolist() == [-1] * 8 + [6, 6]


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
        assert hasattr(lib_mod.load(), name), name
    assert lib_mod.missing_symbols() == []
    assert lib_mod.query("ecm_abi_version") >= 14
    assert len(lib_mod.PROTOTYPES["ecm_disp_splat_fwd"][1]) == 7


def test_max_width_needs_no_gpu(lib_mod):
    import ecm_amd
    k = kernel_constants()
    assert ecm_amd.ops.disparity_splat_max_width() == lib_mod.query("ecm_disp_splat_max_width") == k["MAX_W"]
    assert k["MAX_W"] <= COLS and k["THREADS"] == 256 and k["GRID"] == 512      # splat_t's packing covers every width the op takes


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    lib = lib_mod.load()
    assert lib.ecm_disp_splat_fwd(None, None, None, 1, 1, 1, None) == -1
    p, q = C.c_void_p(64), C.c_void_p(4096)                              # never dereferenced: every call below returns first
    assert lib.ecm_disp_splat_fwd(p, None, None, 1, 1, 8, None) == -1
    assert lib.ecm_disp_splat_fwd(p, p, None, 1, 1, 8, None) == -1        # in place
    for B, H, W in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (-1, 1, 8)):
        assert lib.ecm_disp_splat_fwd(p, q, None, B, H, W, None) == -1
    wide = lib_mod.query("ecm_disp_splat_max_width") + 1
    assert lib.ecm_disp_splat_fwd(p, q, None, 1, 1, wide, None) == -2
    assert lib.ecm_disp_splat_fwd(p, q, None, 1 << 16, 1 << 15, 8, None) == -2          # B * H = 2^31 rows


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
def test_op_refusals():
    import ecm_amd
    ops = ecm_amd.ops
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_splat(torch.zeros(1, 4, 8))
    sig = inspect.signature(ops.disparity_splat)
    assert list(sig.parameters) == ["disp", "with_source"] and sig.parameters["with_source"].default is False

    class OnDevice(torch.Tensor):
        """A CPU tensor that says it is on the device: the shape and dtype contract is checked before anything is launched."""
        is_cuda = True

    fake = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)     # noqa: E731
    for bad in (fake(4, 8), fake(1, 2, 4, 8), fake(2, 1, 1, 4, 8), fake(8)):
        with pytest.raises(RuntimeError, match="disparity_splat"):
            ops.disparity_splat(bad)
    for bad in (fake(1, 0, 8), fake(0, 4, 8), fake(1, 4, 0), fake(1, 1, 0, 8)):
        with pytest.raises(RuntimeError, match="disparity_splat"):
            ops.disparity_splat(bad)
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match="fp32"):
            ops.disparity_splat(fake(1, 4, 8, dtype=dtype))


def test_occlusion_check_is_wired_and_refuses_on_the_cpu():
    import ecm_amd
    from ecm_amd import models
    assert models.CHECKS == ("cross", "splat") and models._CHECK == "cross"
    sig = inspect.signature(models._ECMNet.self_check)
    assert list(sig.parameters) == ["self", "left", "right", "threshold", "rel", "head"]
    assert [sig.parameters[n].default for n in ("threshold", "rel", "head")] == [1.0, 0.0, 2]
    for bad in ("both", "", None, 0, "Cross"):
        with pytest.raises(ValueError, match="check"):
            with models.occlusion_check(bad):
                raise AssertionError("the block was entered")
        assert models._CHECK == "cross"
    with models.occlusion_check("splat"):
        assert models._CHECK == "splat"
        with models.occlusion_check("cross"):
            assert models._CHECK == "cross"
        assert models._CHECK == "splat"
        with pytest.raises(KeyError):
            with models.occlusion_check("cross"):
                raise KeyError("restored on an exception too")
        assert models._CHECK == "splat"
    assert models._CHECK == "cross"
    x = torch.zeros(1, 3, 64, 128)                                       # CPU tensors: a forward on them raises RuntimeError
    for arch in ("cmfsm", "cmf", "cmfsm_sub_8"):
        net = ecm_amd.get_model(arch)
        for bad in (-1, 3, True):
            with pytest.raises(ValueError, match="head"):
                net.self_check(x, x, head=bad)
        with pytest.raises(ValueError, match="threshold"):
            net.self_check(x, x, threshold=-1.0)
        with pytest.raises(RuntimeError):
            net.self_check(x, x)
        with models.occlusion_check("splat"):                            # the refusals of the chains come first in the block as well
            with pytest.raises(ValueError, match="lam"):
                net.smooth(x, x, lam=0.0)
            with pytest.raises(ValueError, match="head"):
                net.refine(x, x, head=3)
    assert all(hasattr(cls, "self_check") for cls in models._MODELS.values())
