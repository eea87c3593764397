"""The disparity post-filters, the part that needs no GPU: `median_t` and `bilateral_t` below, torch
restatements of the definitions at any dtype and on any device -- the references of tests/test_hip_disp_filter.py -- checked in
fp64 against closed forms; the ABI additions; the refusals of ops.disparity_median, ops.disparity_bilateral and refine that come
before any device work; and the conditions under which the GPU test's float cases may be compared with fp64 at all.

Definitions.  A sample q is usable iff it lies inside the image, d[q] is finite and valid[q] != 0 (valid None: all ones); windows
are clipped to the image.  Median, radius r: m = the usable samples of the (2r+1)^2 window, median = the value of rank
floor((m-1)/2) (0-based, ascending) among them, 0 where m == 0; support = m.  Bilateral: for a usable q = p + (dx, dy),
w = exp(-(dx^2 + dy^2) / (2 ss^2) - sum_c (g_c[p] - g_c[q])^2 / (2 sc^2)), excluded where the exponent is NaN;
refined = sum w d / sum w where sum w > 0 else 0; weight = sum w."""
import inspect
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

NEW_ENTRIES = ("ecm_disp_median_fwd", "ecm_disp_bilateral_fwd", "ecm_disp_filter_max_radius")
INF, NAN = float("inf"), float("nan")
K, FLOOR = 4, 2e-7                     # the yardstick of sections 14-17: |out - out64| <= K e32 + FLOOR max|out64|


def kernel_constants():
    """The namespace-level constexpr ints of csrc/disp_filter.hip by name (the GPU test places its shapes at the tile edges)."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "disp_filter.hip")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr):
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


KC = kernel_constants()


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def offsets(r):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def shifted(t, dy, dx):
    """(t gathered at (y + dy, x + dx) with the indices clamped into the image, bool [H,W]: the position is inside the image)."""
    H, W = t.shape[-2:]
    ys, xs = torch.arange(H, device=t.device) + dy, torch.arange(W, device=t.device) + dx
    inside = ((ys >= 0) & (ys < H)).view(H, 1) & ((xs >= 0) & (xs < W)).view(1, W)
    return t.index_select(-2, ys.clamp(0, H - 1)).index_select(-1, xs.clamp(0, W - 1)), inside


def usable_t(d, valid):
    ok = torch.isfinite(d)
    return ok if valid is None else ok & (valid != 0)


def median_t(d, valid, r):
    """(median, support) of d [B,H,W] in its own dtype; valid None or a [B,H,W] mask."""
    ok = usable_t(d, valid)
    vals, oks = [], []
    for dy, dx in offsets(r):
        v, inside = shifted(d, dy, dx)
        o, _ = shifted(ok, dy, dx)
        vals.append(v)
        oks.append(o & inside)
    vals, oks = torch.stack(vals), torch.stack(oks)
    m = oks.sum(0)
    ordered = torch.where(oks, vals, torch.full_like(vals, INF)).sort(0).values
    med = ordered.gather(0, ((m - 1) // 2).clamp(min=0).unsqueeze(0))[0]
    return torch.where(m > 0, med, torch.zeros_like(med)), m.to(d.dtype)


def bilateral_t(d, valid, g, r, ss, sc, reverse=False, base2=False, with_exponent=False):
    """(refined, weight) of d [B,H,W] guided by g [B,C,H,W], in d's dtype.  reverse: the window summed in the opposite order;
    base2: exp2 of the exponent scaled by log2(e) (two variants an fp32 implementation is free to choose).  with_exponent: also
    the smallest exponent of a usable sample."""
    ok = usable_t(d, valid)
    sw, swd = torch.zeros_like(d), torch.zeros_like(d)
    low = INF
    offs = offsets(r)
    for dy, dx in (reversed(offs) if reverse else offs):
        dq, inside = shifted(d, dy, dx)
        oq, _ = shifted(ok, dy, dx)
        gq, _ = shifted(g, dy, dx)
        e = -(dx * dx + dy * dy) / (2 * ss * ss) - ((g - gq) ** 2).sum(1) / (2 * sc * sc)
        keep = oq & inside & ~torch.isnan(e)
        if with_exponent and bool(keep.any()):
            low = min(low, float(e[keep].min()))
        w = torch.exp2(e * math.log2(math.e)) if base2 else torch.exp(e)
        w = torch.where(keep, w, torch.zeros_like(w))
        sw = sw + w
        swd = swd + w * torch.where(keep, dq, torch.zeros_like(dq))
    refined = torch.where(sw > 0, swd / torch.where(sw > 0, sw, torch.ones_like(sw)), torch.zeros_like(sw))
    return (refined, sw, low) if with_exponent else (refined, sw)


# ---- the float cases of the GPU test ----------------------------------------------------------------------------------------------------
# (name, seed, (B, H, W), C, r, sigma_space, sigma_color)
FLOAT_CASES = [
    ("2x9x200_r4", 1801, (2, 9, 200), 3, 4, 2.0, 0.25),
    ("2x9x200_r4_c1", 1802, (2, 9, 200), 1, 4, 2.0, 0.25),
    ("1x7x130_rmax", 1803, (1, 7, 130), 3, KC["R_MAX"], KC["R_MAX"] / 2, 0.5),
    ("1x5x70_r1", 1804, (1, 5, 70), 3, 1, 0.5, 0.25),
    ("tile_r2", 1805, (1, KC["TH"] + 1, 2 * KC["TW"] + 1), 3, 2, 1.0, 0.25),
]
FLOAT_IDS = [c[0] for c in FLOAT_CASES]


def float_case(seed, shape, C):
    """(d, valid, guide) in fp32 on the CPU: every row of d a ramp with a 15 px step at mid-width plus 0.5 px of noise, the guide
    0.3 U(0,1) plus 0.6 on the far side of the step, a random 30 % of the pixels invalid."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    far = (x >= W // 2).float()
    a = 5 + 10 * torch.rand(B, H, 1, generator=gen)
    slope = 10 * torch.rand(B, H, 1, generator=gen) / W
    d = a + slope * x + 15 * far + 0.5 * torch.rand(B, H, W, generator=gen)
    guide = 0.3 * torch.rand(B, C, H, W, generator=gen) + 0.6 * far.view(1, 1, 1, W)
    valid = torch.rand(B, H, W, generator=gen) >= 0.3
    return d.contiguous(), valid, guide.contiguous()


@pytest.mark.parametrize("name,seed,shape,C,r,ss,sc", FLOAT_CASES, ids=FLOAT_IDS)
def test_float_cases_can_be_compared_with_fp64(name, seed, shape, C, r, ss, sc):
    d, valid, g = float_case(seed, shape, C)
    assert 0 <= float(g.min()) and float(g.max()) <= 0.9 and sc >= 0.25 and r * r / (ss * ss) <= 8 and r <= KC["R_MAX"]
    r32, w32, low32 = bilateral_t(d, valid, g, r, ss, sc, with_exponent=True)
    r64, w64, low64 = bilateral_t(d.double(), valid, g.double(), r, ss, sc, with_exponent=True)
    # no fp32 weight underflows (exp(-60) = 9e-27 is far above the smallest normal fp32, 1.2e-38), so sum w > 0 is decided
    # alike in fp32 and fp64 ...
    assert min(low32, low64) > -60
    # ... and with the guide in [0, 0.9]: r^2 / ss^2 + C 0.81 / (2 sc^2) <= 8 + 19.44 for C = 3
    assert min(low32, low64) > -36
    assert int((w32 == 0).sum()) == int((w64 == 0).sum())
    assert 0.25 < 1 - float(valid.float().mean()) < 0.35 and bool((w64 > 0).any())
    # an fp32 implementation that sums the other way round and uses exp2 stays inside the yardstick: there is room for a
    # kernel's own order, but not for a wrong one
    worst = 0.0
    for got, want, plain in zip(bilateral_t(d, valid, g, r, ss, sc, reverse=True, base2=True), (r64, w64), (r32, w32)):
        bound = K * float((plain.double() - want).abs().max()) + FLOOR * float(want.abs().max())
        worst = max(worst, float((got.double() - want).abs().max()) / bound)
    print(f"DFVARIANT {name} {worst:.3f}")
    assert worst <= 1.0


# ---- closed forms of the median, fp64 -----------------------------------------------------------------------------------------------
RADII = (1, 2, 3)


def clipped_count(n, r):
    """[n]: how many of the 2r+1 positions about each index lie in [0, n)."""
    i = torch.arange(n)
    return (i + r).clamp(max=n - 1) - (i - r).clamp(min=0) + 1


@pytest.mark.parametrize("r", RADII)
def test_median_of_a_constant_plane(r):
    d = torch.full((2, 5, 9), 3.25, dtype=torch.float64)
    med, sup = median_t(d, None, r)
    assert torch.equal(med, d)
    assert torch.equal(sup, (clipped_count(5, r).view(5, 1) * clipped_count(9, r).view(1, 9)).double().expand(2, 5, 9))
    med1, sup1 = median_t(d, torch.ones(2, 5, 9, dtype=torch.uint8), r)
    assert torch.equal(med1, med) and torch.equal(sup1, sup)


@pytest.mark.parametrize("r", RADII)
def test_median_of_a_ramp_along_x(r):
    H, W = 6, 12
    d = torch.arange(W, dtype=torch.float64).expand(1, H, W).contiguous()
    med, _ = median_t(d, None, r)
    assert torch.equal(med[..., r:W - r], d[..., r:W - r])             # a full window: 2r+1 columns, k rows each: the middle one
    # a border column sees c = r + 1 columns, each value k times (k the rows in view): rank floor((k c - 1) / 2) lies in column
    # (c - 1) // 2 of them for every k >= 1 -- the LOWER of the two middle columns where c is even
    shift = (r + 1 - 1) // 2
    assert bool((med[..., 0] == shift).all()) and bool((med[..., W - 1] == W - 1 - r + shift).all())
    assert shift == r // 2 and (r % 2 == 0 or W - 1 - r + shift < W - 1 - r / 2)      # odd r: below the window's centre


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("spike", [100.0, -5.0])
def test_median_removes_a_lone_impulse(r, spike):
    for at in ((4, 5), (0, 0), (8, 10), (0, 6)):
        d = torch.full((1, 9, 11), 2.0, dtype=torch.float64)
        d[0][at] = spike
        med, _ = median_t(d, None, r)
        assert bool((med == 2.0).all())


@pytest.mark.parametrize("r", RADII)
def test_median_is_the_lower_one_under_a_checkerboard(r):
    H, W = 7, 9
    d = (torch.arange(H * W, dtype=torch.float64).view(1, H, W) * 7) % 64        # distinct enough, unsorted
    valid = ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2 == 0).view(1, H, W)
    med, sup = median_t(d, valid, r)
    even = upper_differs = 0
    for y in range(H):
        for x in range(W):
            vals = sorted(float(d[0, yy, xx]) for yy in range(max(0, y - r), min(H, y + r + 1))
                          for xx in range(max(0, x - r), min(W, x + r + 1)) if valid[0, yy, xx])
            m = len(vals)
            assert sup[0, y, x] == m and med[0, y, x] == vals[(m - 1) // 2]
            even += m % 2 == 0
            upper_differs += m % 2 == 0 and vals[m // 2] != vals[(m - 1) // 2]
    assert even > 0 and upper_differs > 0 and even < H * W


@pytest.mark.parametrize("r", RADII)
def test_median_of_nothing_and_of_one(r):
    H, W = 8, 10
    d = torch.rand(1, H, W, dtype=torch.float64) + 1
    med, sup = median_t(d, torch.zeros(1, H, W, dtype=torch.uint8), r)
    assert bool((med == 0).all()) and bool((sup == 0).all())
    for y0, x0 in ((0, 0), (H - 1, W - 1), (3, 4)):
        valid = torch.zeros(1, H, W, dtype=torch.bool)
        valid[0, y0, x0] = True
        med, sup = median_t(d, valid, r)
        near = ((torch.arange(H).view(H, 1) - y0).abs() <= r) & ((torch.arange(W).view(1, W) - x0).abs() <= r)
        assert torch.equal(sup[0], near.double()) and torch.equal(med[0], torch.where(near, d[0, y0, x0], 0.0).double())


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_median_leaves_non_finite_values_out(r, bad):
    H, W = 7, 8
    d = torch.full((1, H, W), 2.0, dtype=torch.float64)
    d[0, 3, 4] = bad
    d[0, 0, 0] = bad
    med, sup = median_t(d, None, r)
    clean = median_t(torch.full((1, H, W), 2.0, dtype=torch.float64), None, r)[1]
    near = lambda y0, x0: (((torch.arange(H).view(H, 1) - y0).abs() <= r) & ((torch.arange(W).view(1, W) - x0).abs() <= r)).double()   # noqa: E731
    assert bool((med == 2.0).all()) and torch.equal(sup[0], clean[0] - near(3, 4) - near(0, 0))


# ---- closed forms of the bilateral filter, fp64 -------------------------------------------------------------------------------------------
def test_bilateral_of_a_constant_plane():
    gen = torch.Generator().manual_seed(3)
    d = torch.full((2, 6, 9), 7.5, dtype=torch.float64)
    for C in (1, 3, 4):
        g = torch.rand(2, C, 6, 9, generator=gen, dtype=torch.float64)
        for r in (1, 3, KC["R_MAX"]):
            refined, weight = bilateral_t(d, None, g, r, 2.0, 0.25)
            assert float((refined - 7.5).abs().max()) <= 1e-14 and bool((weight >= 1).all())


def test_bilateral_with_a_constant_guide_is_a_gaussian_blur():
    W, ss = 9, 0.8
    gen = torch.Generator().manual_seed(4)
    d = torch.rand(1, 1, W, generator=gen, dtype=torch.float64) * 10
    g = torch.full((1, 2, 1, W), 0.4, dtype=torch.float64)
    refined, weight = bilateral_t(d, None, g, 1, ss, 0.1)
    e = math.exp(-1 / (2 * ss * ss))
    a, b, c = d[0, 0, :-2], d[0, 0, 1:-1], d[0, 0, 2:]
    assert float((refined[0, 0, 1:-1] - (a * e + b + c * e) / (1 + 2 * e)).abs().max()) <= 1e-14
    assert float((weight[0, 0, 1:-1] - (1 + 2 * e)).abs().max()) <= 1e-14
    assert abs(float(refined[0, 0, 0]) - float((d[0, 0, 0] + e * d[0, 0, 1]) / (1 + e))) <= 1e-14      # clipped, not padded


@pytest.mark.parametrize("r", [1, 4])
def test_bilateral_keeps_a_step_that_the_guide_has_too(r):
    H, W, dd, dg, sc = 9, 20, 15.0, 0.9, 0.2
    far = (torch.arange(W) >= W // 2).double().expand(1, H, W)
    d = 4.0 + dd * far
    g = (dg * far).unsqueeze(1).contiguous()
    refined, _ = bilateral_t(d.contiguous(), None, g, r, 2.0, sc)
    # a pixel's own side weighs >= 1 (the centre), the other side at most n exp(-dg^2 / (2 sc^2)) in all
    cap = dd * (2 * r + 1) ** 2 * math.exp(-dg * dg / (2 * sc * sc))
    assert cap < 1.0 and float((refined - d).abs().max()) <= cap and float((refined - d).abs().max()) > 0


def test_bilateral_fills_a_zero_row_from_its_neighbours():
    d = torch.full((1, 7, 12), 5.0, dtype=torch.float64)
    d[0, 3] = 0
    g = torch.rand(1, 3, 7, 12, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    refined, weight = bilateral_t(d, d > 0, g, 2, 2.0, 0.5)
    assert float((refined - 5.0).abs().max()) <= 1e-14 and bool((weight > 0).all())
    same_guide = bilateral_t(d, d > 0, torch.zeros(1, 1, 7, 12, dtype=torch.float64), 1, 2.0, 0.5)[1]
    e = math.exp(-1 / 8)                                               # the row itself adds nothing: 6 of the 9 weights remain
    assert abs(float(same_guide[0, 3, 5]) - (2 * e + 4 * e * e)) <= 1e-14 and abs(float(same_guide[0, 5, 5]) - (1 + 4 * e + 4 * e * e)) <= 1e-14


def test_bilateral_leaves_out_a_sample_whose_guide_is_nan_and_weighs_a_lone_centre_one():
    gen = torch.Generator().manual_seed(6)
    d = torch.rand(1, 6, 8, generator=gen, dtype=torch.float64) * 20
    g = torch.rand(1, 3, 6, 8, generator=gen, dtype=torch.float64)
    holed, masked = g.clone(), torch.ones(1, 6, 8, dtype=torch.bool)
    holed[0, 1, 2, 5] = NAN
    masked[0, 2, 5] = False
    got, want = bilateral_t(d, None, holed, 2, 2.0, 0.25), bilateral_t(d, masked, g, 2, 2.0, 0.25)
    elsewhere = masked.clone()
    assert all(torch.equal(a[elsewhere], b[elsewhere]) for a, b in zip(got, want))
    assert got[0][0, 2, 5] == 0 and got[1][0, 2, 5] == 0              # every exponent of that window is NaN
    lone = torch.zeros(1, 6, 8, dtype=torch.bool)
    lone[0, 4, 1] = True
    refined, weight = bilateral_t(d, lone, g, 2, 2.0, 0.25)
    assert weight[0, 4, 1] == 1 and refined[0, 4, 1] == d[0, 4, 1]
    assert int((weight > 0).sum()) == 4 * 4                            # its 5 x 5 neighbourhood clipped: rows 2..5, columns 0..3
    assert bool((weight[0, 2:6, 0:4] > 0).all())


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
    assert lib_mod.query("ecm_abi_version") >= 11
    assert len(lib_mod.PROTOTYPES["ecm_disp_median_fwd"][1]) == 8 and len(lib_mod.PROTOTYPES["ecm_disp_bilateral_fwd"][1]) == 12


def test_max_radius_needs_no_gpu(lib_mod):
    import ecm_amd
    assert lib_mod.query("ecm_disp_filter_max_radius", 0) == 3 == KC["MEDIAN_R_MAX"]
    assert lib_mod.query("ecm_disp_filter_max_radius", 1) == KC["R_MAX"] >= 4
    assert lib_mod.query("ecm_disp_filter_max_radius", 2) == -1 and lib_mod.query("ecm_disp_filter_max_radius", -1) == -1
    assert ecm_amd.ops.disp_filter_max_radius("median") == 3 and ecm_amd.ops.disp_filter_max_radius("bilateral") == KC["R_MAX"]
    with pytest.raises(ValueError):
        ecm_amd.ops.disp_filter_max_radius("box")
    assert KC["TW"] == KC["WAVE"] == 64 and KC["THREADS"] == 256 and KC["TH"] % KC["NWAVE"] == 0
    # the bilateral kernel's LDS at the largest radius and C = 4 stays under the 64 KB a kernel has without asking
    r = KC["R_MAX"]
    assert ((1 + KC["C_MAX"]) * (KC["TH"] + 2 * r) * (KC["TW"] + 2 * r) + 2 * r + 1) * 4 <= 64 * 1024


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    import ctypes as C
    lib = lib_mod.load()
    p = C.c_void_p(64)                                                 # never dereferenced: every call below returns first
    med, bil = lib.ecm_disp_median_fwd, lib.ecm_disp_bilateral_fwd
    assert med(None, None, None, 1, 1, 1, 1, None) == -1
    assert med(None, p, p, 1, 4, 4, 1, None) == -1 and med(p, p, None, 1, 4, 4, 1, None) == -1
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert med(p, None, p, B, H, W, 1, None) == -1
        assert bil(p, None, p, p, B, 3, H, W, 1, 1.0, 1.0, None) == -1
    for radius in (0, -1, 4, 100):
        assert med(p, None, p, 1, 4, 4, radius, None) == -1
    assert bil(None, None, None, None, 1, 1, 1, 1, 1, 1.0, 1.0, None) == -1
    assert bil(p, p, None, p, 1, 3, 4, 4, 1, 1.0, 1.0, None) == -1 and bil(p, p, p, None, 1, 3, 4, 4, 1, 1.0, 1.0, None) == -1
    for radius in (0, -1, KC["R_MAX"] + 1):
        assert bil(p, None, p, p, 1, 3, 4, 4, radius, 1.0, 1.0, None) == -1
    for channels in (0, 5, -1):
        assert bil(p, None, p, p, 1, channels, 4, 4, 1, 1.0, 1.0, None) == -1
    for sigma in (0.0, -1.0, NAN, INF, -INF):
        assert bil(p, None, p, p, 1, 3, 4, 4, 1, sigma, 1.0, None) == -1
        assert bil(p, None, p, p, 1, 3, 4, 4, 1, 1.0, sigma, None) == -1
    assert med(p, None, p, 1 << 11, 1 << 10, 1 << 10, 1, None) == -2                # B H W = 2^31
    assert bil(p, None, p, p, 1 << 11, 3, 1 << 10, 1 << 10, 1, 1.0, 1.0, None) == -2


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
def test_op_refusals():
    import ecm_amd
    ops = ecm_amd.ops
    d, g = torch.zeros(1, 4, 8), torch.zeros(1, 3, 4, 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_median(d)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_bilateral(d, g)
    for bad in (0, 4, -1, 1.0, None, True, "2"):
        with pytest.raises(ValueError, match="radius"):
            ops.disparity_median(d, radius=bad)
    for bad in (0, ops.disp_filter_max_radius("bilateral") + 1, 2.0, None, True):
        with pytest.raises(ValueError, match="radius"):
            ops.disparity_bilateral(d, g, radius=bad)
    for bad in (0.0, -1.0, NAN, INF, None, "1", True):
        with pytest.raises(ValueError, match="sigma_space"):
            ops.disparity_bilateral(d, g, sigma_space=bad)
        with pytest.raises(ValueError, match="sigma_color"):
            ops.disparity_bilateral(d, g, sigma_color=bad)
    assert ops.check_median_radius(3) == 3 and ops.check_bilateral_parameters(4, 2, 1) == (4, 2.0, 1.0)
    sig = inspect.signature(ops.disparity_median)
    assert list(sig.parameters) == ["disp", "valid", "radius", "with_support"]
    assert [sig.parameters[n].default for n in ("valid", "radius", "with_support")] == [None, 2, False]
    sig = inspect.signature(ops.disparity_bilateral)
    assert list(sig.parameters) == ["disp", "guide", "valid", "radius", "sigma_space", "sigma_color", "with_weight"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [None, 4, 2.0, 0.25, False]


def test_refine_is_wired_and_refuses_on_the_cpu():
    import ecm_amd
    from ecm_amd import models
    assert models.Refined._fields == models.CrossCheck._fields + ("median", "refined")
    sig = inspect.signature(models._ECMNet.refine)
    assert list(sig.parameters) == ["self", "left", "right", "threshold", "rel", "head", "median_radius", "bilateral_radius",
                                    "sigma_space", "sigma_color"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [1.0, 0.0, 2, 2, 4, 2.0, 0.25]
    x = torch.zeros(1, 3, 64, 128)
    for name in ("cmfsm", "cmfsm_sub_8"):
        net = ecm_amd.get_model(name)
        for kw, what in (({"head": 3}, "head"), ({"threshold": -1.0}, "threshold"), ({"rel": INF}, "rel"),
                         ({"median_radius": 0}, "radius"), ({"median_radius": 4}, "radius"), ({"median_radius": 2.0}, "radius"),
                         ({"bilateral_radius": 0}, "radius"), ({"bilateral_radius": 99}, "radius"),
                         ({"sigma_space": 0.0}, "sigma_space"), ({"sigma_color": NAN}, "sigma_color")):
            with pytest.raises(ValueError, match=what):
                net.refine(x, x, **kw)
        with pytest.raises(RuntimeError):
            net.refine(x, x)
        with pytest.raises(RuntimeError):
            net.refine(x, x, median_radius=None, bilateral_radius=None)
    assert all(hasattr(cls, "refine") for cls in models._MODELS.values())
