"""The WLS disparity smoother, the part that needs no GPU: `wls_t` below, the torch restatement of the
definition at any dtype and on any device -- the reference of tests/test_hip_disp_wls.py -- checked in fp64 against a dense solve
and against closed forms; the ABI additions; the refusals of ops.disparity_wls and smooth that come before any device work; and
the conditions under which the GPU test's float cases may be compared with fp64 at all.

Definition.  A pixel is usable iff d and conf are finite and conf >= 0 (conf None: all ones); elsewhere both count as 0.  Link
weight between 4-neighbours p, q: w = exp(-sqrt(sum_c (g_c[p] - g_c[q])^2) / sigma_color), 0 where that is NaN.  A line solve is
(I + L A) u = f with a_i = -L w_{i-1}, c_i = -L w_i, b_i = 1 - a_i - c_i by the Thomas algorithm in natural order.  N = conf d and
D = conf go through, for t = 1..T with L_t = 1.5 4^(T-t) / (4^T - 1) lam, every row and then every column; smoothed = N / D where
D > 0 else 0, weight = D."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

NEW_ENTRIES = ("ecm_disp_wls_fwd", "ecm_disp_wls_scratch_bytes")
INF, NAN = float("inf"), float("nan")
K, FLOOR = 4, 2e-7                     # the yardstick of sections 14-19: |out - out64| <= K e32 + FLOOR max|out64|
D_FLOOR = 1e-25                        # a D64 that is not exactly 0 is at least this: far above the smallest normal fp32


def kernel_constants():
    """The namespace-level constexpr ints of csrc/disp_wls.hip by name (the GPU test places its shapes at the tile edges)."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "disp_wls.hip")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr):
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


KC = kernel_constants()


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def link_weights_t(g, sigma_color):
    """(horizontal [B,H,W-1], vertical [B,H-1,W]) link weights of the guide g [B,C,H,W], in g's dtype."""
    def w(a, b):
        e = torch.exp(-torch.sqrt(((a - b) ** 2).sum(1)) / sigma_color)
        return torch.where(torch.isnan(e), torch.zeros_like(e), e)
    return w(g[:, :, :, :-1], g[:, :, :, 1:]), w(g[:, :, :-1, :], g[:, :, 1:, :])


def thomas(f, w, lam_t):
    """(I + lam_t A) u = f along the last dimension: f [..., n], w [..., n-1] (broadcast against f), natural order."""
    n = f.shape[-1]
    if n == 1:
        return f.clone()
    lw = (-lam_t * w).expand(f.shape[:-1] + (n - 1,))
    zero = torch.zeros_like(f[..., :1])
    a, c = torch.cat([zero, lw], -1), torch.cat([lw, zero], -1)
    b = 1 - a - c
    cp, fp = [], []
    c_prev = f_prev = zero[..., 0]
    for i in range(n):
        den = b[..., i] - a[..., i] * c_prev
        c_prev = c[..., i] / den
        f_prev = (f[..., i] - a[..., i] * f_prev) / den
        cp.append(c_prev)
        fp.append(f_prev)
    u, u_next = [None] * n, zero[..., 0]
    for i in reversed(range(n)):
        u_next = u[i] = fp[i] - cp[i] * u_next
    return torch.stack(u, -1)


def lam_of(t, T, lam):
    return 1.5 * 4 ** (T - t) / (4 ** T - 1) * lam


def planes_t(d, conf):
    """(N, D) at the start: conf * d and conf over the usable pixels, 0 elsewhere."""
    conf = torch.ones_like(d) if conf is None else conf.to(d.dtype)
    ok = torch.isfinite(d) & torch.isfinite(conf) & (conf >= 0)
    zero = torch.zeros_like(d)
    conf = torch.where(ok, conf, zero)
    return conf * torch.where(ok, d, zero), conf


def wls_t(d, g, conf, lam, sigma_color, iterations):
    """(smoothed, weight) of d [B,H,W] guided by g [B,C,H,W] under conf [B,H,W] or None, in d's dtype on d's device."""
    wh, wv = link_weights_t(g.to(d.dtype), sigma_color)
    nd = torch.stack(planes_t(d, conf))                                # N and D: the same instructions, the same coefficients
    for t in range(1, iterations + 1):
        lam_t = lam_of(t, iterations, lam)
        nd = thomas(nd, wh, lam_t)
        nd = thomas(nd.transpose(-1, -2), wv.transpose(-1, -2), lam_t).transpose(-1, -2)
    n, dd = nd[0].contiguous(), nd[1].contiguous()
    pos = dd > 0
    return torch.where(pos, n / torch.where(pos, dd, torch.ones_like(dd)), torch.zeros_like(n)), dd


# ---- the float cases of the GPU test ----------------------------------------------------------------------------------------------------
# (name, seed, (B, H, W), C, lam, sigma_color, T, share of the pixels with a nonzero confidence)
FLOAT_CASES = [
    ("2x9x70_lam8", 2001, (2, 9, 70), 3, 8.0, 0.25, 3, 0.3),
    ("1x33x65_lam128_c1", 2002, (1, 33, 65), 1, 128.0, 0.1, 3, 0.05),
    ("1x65x130_lam8000_c4", 2003, (1, 65, 130), 4, 8000.0, 0.5, 3, 0.02),
    ("1x5x200_lam1", 2004, (1, 5, 200), 3, 1.0, 0.05, 2, 0.5),
    ("1x64x64_lam8000_t4", 2005, (1, 64, 64), 3, 8000.0, 1.0, 4, 0.1),
]
FLOAT_IDS = [c[0] for c in FLOAT_CASES]


def float_case(seed, shape, C, sigma_color, share):
    """(d, guide, conf) in fp32 on the CPU: every row of d a ramp with a 15 px step at mid-width plus 0.5 px of noise (values up
    to 40), the guide 0.4 sigma_color U(0,1) plus 0.6 on the far side of the step -- a link inside a side keeps a weight of at
    least exp(-0.4 sqrt(C)), so D does not underflow on the way from one confident pixel to the next --, conf uniform in (0,1)
    on a random `share` of the pixels and 0 on the rest."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    far = (x >= W // 2).float()
    a = 5 + 10 * torch.rand(B, H, 1, generator=gen)
    slope = 10 * torch.rand(B, H, 1, generator=gen) / W
    d = a + slope * x + 15 * far + 0.5 * torch.rand(B, H, W, generator=gen)
    guide = 0.4 * sigma_color * torch.rand(B, C, H, W, generator=gen) + 0.6 * far.view(1, 1, 1, W)
    u = torch.rand(B, H, W, generator=gen)
    conf = torch.where(torch.rand(B, H, W, generator=gen) < share, 0.001 + 0.998 * u, torch.zeros(()))
    return d.contiguous(), guide.contiguous(), conf.contiguous()


def sparse_conf(shape, seed, share=0.3):
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(shape, generator=gen)
    return torch.where(torch.rand(shape, generator=gen) < share, 0.001 + 0.998 * u, torch.zeros(()))


@pytest.mark.parametrize("name,seed,shape,C,lam,sc,T,share", FLOAT_CASES, ids=FLOAT_IDS)
def test_float_cases_can_be_compared_with_fp64(name, seed, shape, C, lam, sc, T, share):
    d, g, conf = float_case(seed, shape, C, sc, share)
    nonzero = float((conf > 0).float().mean())
    assert 0.02 <= nonzero <= 0.5 and float(conf.max()) < 1 and float(d.max()) <= 40.5 and float(d.min()) >= 5
    s32, w32 = wls_t(d, g, conf, lam, sc, T)
    s64, w64 = wls_t(d.double(), g.double(), conf.double(), lam, sc, T)
    # D > 0 is decided alike in fp32 and fp64: no D64 is so small that an fp32 D could have underflowed to 0
    tiny = w64[w64 != 0]
    print(f"WLSCASE {name} nonzero {nonzero:.3f} min D64 {float(tiny.min()):.3e} e32 {float((s32.double() - s64).abs().max()):.3e}")
    assert bool((w64 >= 0).all()) and float(tiny.min()) >= D_FLOOR
    assert torch.equal(w32 == 0, w64 == 0) and torch.equal(s32 == 0, s64 == 0)
    assert bool(torch.isfinite(s32).all()) and bool(torch.isfinite(w32).all())
    sure = conf > 0
    assert float(s64.min()) >= float(d[sure].min()) - 1e-9 and float(s64.max()) <= float(d[sure].max()) + 1e-9


# ---- one line solve against the dense matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7])
def test_thomas_equals_the_dense_solve(n):
    gen = torch.Generator().manual_seed(n)
    f = torch.rand(3, n, generator=gen, dtype=torch.float64) * 10
    w = torch.rand(3, max(n - 1, 0), generator=gen, dtype=torch.float64)
    lam_t = 5.5
    u = thomas(f, w, lam_t)
    for r in range(3):
        m = np.eye(n)
        for i in range(n - 1):
            lw = lam_t * float(w[r, i])
            m[i, i] += lw
            m[i + 1, i + 1] += lw
            m[i, i + 1] -= lw
            m[i + 1, i] -= lw
        want = np.linalg.solve(m, f[r].numpy())
        assert float(np.abs(u[r].numpy() - want).max()) <= 1e-12
    if n == 1:
        assert torch.equal(u, f)


# ---- closed forms, fp64 ---------------------------------------------------------------------------------------------------------------
def some_case(seed, shape=(2, 7, 11), C=3):
    gen = torch.Generator().manual_seed(seed)
    d = 5 + 30 * torch.rand(shape, generator=gen, dtype=torch.float64)
    g = torch.rand(shape[0], C, *shape[1:], generator=gen, dtype=torch.float64)
    return d, g, sparse_conf(shape, seed + 1).double()


@pytest.mark.parametrize("lam,sc,T", [(8.0, 0.25, 3), (8000.0, 1.0, 4), (1.0, 0.05, 1)])
def test_mass_is_conserved(lam, sc, T):
    d, g, conf = some_case(31)
    s, w = wls_t(d, g, conf, lam, sc, T)
    assert abs(float(w.sum()) - float(conf.sum())) <= 1e-10 * float(conf.sum())
    assert abs(float((s * w).sum()) - float((conf * d).sum())) <= 1e-10 * float((conf * d).sum())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("value", [16.0, 0.5])
def test_a_constant_power_of_two_plane_returns_itself_exactly(dtype, value):
    _, g, conf = some_case(32)
    d = torch.full(conf.shape, value, dtype=dtype)
    for c in (None, conf.to(dtype), (conf > 0).to(dtype)):
        s, w = wls_t(d, g.to(dtype), c, 64.0, 0.25, 3)
        assert bool((w > 0).any()) and bool((s[w > 0] == value).all()) and bool((s[w <= 0] == 0).all())


def test_full_confidence_and_a_constant_guide():
    d, _, _ = some_case(33)
    g = torch.full((2, 2, 7, 11), 0.3, dtype=torch.float64)
    for lam, T in ((8.0, 3), (8000.0, 2)):
        s, w = wls_t(d, g, torch.ones_like(d), lam, 0.25, T)
        assert float((w - 1).abs().max()) <= 1e-12
        assert float(s.min()) >= float(d.min()) - 1e-12 and float(s.max()) <= float(d.max()) + 1e-12
        assert float(s.max() - s.min()) < float(d.max() - d.min())     # and it does smooth
        s0, w0 = wls_t(d, g, None, lam, 0.25, T)
        assert torch.equal(s0, s) and torch.equal(w0, w)


@pytest.mark.parametrize("at", [(0, 0), (6, 10), (3, 4), (0, 10)])
def test_a_single_confident_pixel_spreads_its_value(at):
    d, g, _ = some_case(34, (1, 7, 11))
    for value in (4.0, 3.7):
        conf = torch.zeros_like(d)
        conf[0][at] = 0.6
        d[0][at] = value
        s, w = wls_t(d, g, conf, 32.0, 0.5, 2)
        assert bool((w > 0).all())                                     # every link is open: the whole image hears of it
        assert float((s - value).abs().max()) <= (0 if value == 4.0 else 1e-12)


def test_a_step_that_the_guide_shares_is_kept():
    H, W, sc = 6, 16, 0.02
    far = (torch.arange(W) >= W // 2).double().expand(1, H, W)
    d = (4.0 + 15.0 * far).contiguous()
    g = (0.8 * far).unsqueeze(1).contiguous()                          # 0.8 / 0.02 = 40
    assert 0.8 / sc >= 40
    s, w = wls_t(d, g, None, 8000.0, sc, 3)
    assert float((s - d).abs().max()) <= 1e-6
    blurred, _ = wls_t(d, torch.zeros_like(g), None, 8000.0, sc, 3)    # without the edge in the guide the step is gone
    assert float((blurred - d).abs().max()) > 5


def test_a_nan_column_of_the_guide_cuts_the_image_in_two():
    d, g, conf = some_case(35, (1, 7, 11))
    k = 6
    g[:, 1, :, k] = NAN
    conf[..., k:] = 0
    assert bool((conf[..., :k] > 0).any())
    s, w = wls_t(d, g, conf, 8000.0, 0.25, 3)
    assert bool((w[..., k:] == 0).all()) and bool((s[..., k:] == 0).all())
    assert bool((w[..., :k] > 0).all()) and bool(torch.isfinite(s).all())
    conf[0, 2, k] = 0.5                                                # a confident pixel inside the column stays alone
    s, w = wls_t(d, g, conf, 8000.0, 0.25, 3)
    assert w[0, 2, k] == 0.5 and s[0, 2, k] == d[0, 2, k] and int((w[..., k:] > 0).sum()) == 1


def test_unusable_pixels_count_as_confidence_zero():
    d, g, conf = some_case(36)
    conf = conf.clamp(min=0.05)
    spots = [(0, 0, 0), (0, 3, 4), (1, 6, 10), (1, 2, 2)]
    want_conf = conf.clone()
    for spot in spots:
        want_conf[spot] = 0
    want = wls_t(d, g, want_conf, 8.0, 0.25, 3)
    for bad_d, bad_conf in ((NAN, None), (INF, None), (-INF, None), (None, -0.5), (None, NAN), (None, INF), (None, -INF)):
        dd, cc = d.clone(), conf.clone()
        for spot in spots:
            if bad_d is not None:
                dd[spot] = bad_d
            else:
                cc[spot] = bad_conf
        got = wls_t(dd, g, cc, 8.0, 0.25, 3)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (bad_d, bad_conf)
    got = wls_t(torch.where(want_conf > 0, d, torch.full_like(d, NAN)), g, None, 8.0, 0.25, 3)      # conf None: all ones
    ones = wls_t(d, g, (want_conf > 0).double(), 8.0, 0.25, 3)
    assert torch.equal(got[0], ones[0]) and torch.equal(got[1], ones[1])


def test_one_iteration_is_a_row_solve_then_a_column_solve():
    d, g, conf = some_case(37)
    lam = 12.0
    assert lam_of(1, 1, lam) == 1.5 / 3 * lam and abs(sum(lam_of(t, 3, lam) for t in (1, 2, 3)) - 1.5 * lam / 3) < 1e-12
    wh, wv = link_weights_t(g, 0.25)
    planes = []
    for f in (conf * d, conf):
        f = thomas(f, wh, 0.5 * lam)
        planes.append(thomas(f.transpose(-1, -2), wv.transpose(-1, -2), 0.5 * lam).transpose(-1, -2))
    s, w = wls_t(d, g, conf, lam, 0.25, 1)
    assert torch.equal(w, planes[1]) and torch.equal(s, planes[0] / planes[1])


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
    assert lib_mod.query("ecm_abi_version") >= 13
    assert len(lib_mod.PROTOTYPES["ecm_disp_wls_fwd"][1]) == 13 and len(lib_mod.PROTOTYPES["ecm_disp_wls_scratch_bytes"][1]) == 3


def test_scratch_bytes_needs_no_gpu(lib_mod):
    q = lambda *a: lib_mod.query("ecm_disp_wls_scratch_bytes", *a)     # noqa: E731
    assert q(1, 1, 1) > 0 and q(1, 576, 960) >= 576 * 960 * 4 and q(4, 576, 960) == 4 * q(1, 576, 960)
    assert q(1 << 10, 1 << 10, 1 << 10) >= 1 << 32                     # 64-bit
    assert q(0, 4, 4) < 0 and q(1, 0, 4) < 0 and q(1, 4, -1) < 0
    assert KC["THREADS"] == 256 and KC["LINES"] * KC["CHUNK"] == KC["TILE"] == KC["VLINES"] * KC["VCHUNK"]
    assert KC["TILE"] % KC["THREADS"] == 0 and KC["LINES"] <= 64 and KC["VLINES"] <= 64      # the sweep is lanes of one wave
    assert 3 * KC["LINES"] * (KC["CHUNK"] + KC["PAD"]) * 4 <= 64 * 1024                      # LDS of a pass


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    import ctypes as C
    wls = lib_mod.load().ecm_disp_wls_fwd
    p = C.c_void_p(64)                                                 # never dereferenced: every call below returns first
    good = [p, None, p, p, p, 1, 3, 4, 4, 8.0, 0.25, 3, None]
    for at in (0, 2, 3, 4):                                            # d, guide, out, scratch
        args = list(good)
        args[at] = None
        assert wls(*args) == -1
    for at in (5, 7, 8):                                               # B, H, W
        for bad in (0, -1):
            args = list(good)
            args[at] = bad
            assert wls(*args) == -1
    for at, bads in ((6, (0, 5, -1)), (12 - 1, (0, 9, -1)), (9, (0.0, -1.0, NAN, INF, -INF)), (10, (0.0, -1.0, NAN, INF, -INF))):
        for bad in bads:
            args = list(good)
            args[at] = bad
            assert wls(*args) == -1, (at, bad)
    args = list(good)
    args[5], args[7], args[8] = 1 << 11, 1 << 10, 1 << 10              # B H W = 2^31
    assert wls(*args) == -2


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
def test_op_refusals():
    import ecm_amd
    ops = ecm_amd.ops
    d, g = torch.zeros(1, 4, 8), torch.zeros(1, 3, 4, 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_wls(d, g)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_wls(d, g, torch.ones(1, 4, 8))
    for bad in (0.0, 0, -1.0, NAN, INF, None, "1", True):
        with pytest.raises(ValueError, match="lam"):
            ops.disparity_wls(d, g, lam=bad)
        with pytest.raises(ValueError, match="sigma_color"):
            ops.disparity_wls(d, g, sigma_color=bad)
        with pytest.raises(ValueError, match="sigma_color"):
            ops.check_wls_parameters(8000.0, bad, 3)
    for bad in (0, 9, -1, 2.0, None, True, "3"):
        with pytest.raises(ValueError, match="iterations"):
            ops.disparity_wls(d, g, iterations=bad)
    with pytest.raises(ValueError, match="smooth: lam"):
        ops.check_wls_parameters(0, 0.25, 3, who="smooth")
    assert ops.check_wls_parameters(8, 1, np.int64(8)) == (8.0, 1.0, 8) and ops.check_wls_parameters(0.5, 0.25, 1) == (0.5, 0.25, 1)
    sig = inspect.signature(ops.disparity_wls)
    assert list(sig.parameters) == ["disp", "guide", "confidence", "lam", "sigma_color", "iterations", "with_weight"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [None, 8000.0, 0.25, 3, False]


def test_smooth_is_wired_and_refuses_on_the_cpu():
    import ecm_amd
    from ecm_amd import models
    assert models.Smoothed._fields == models.CrossCheck._fields + ("confidence", "smoothed")
    assert models.Smoothed._fields == ("disparity", "disparity_right", "error", "kind", "filled", "confidence", "smoothed")
    sig = inspect.signature(models._ECMNet.smooth)
    assert list(sig.parameters) == ["self", "left", "right", "threshold", "rel", "head", "speckle_size", "speckle_diff", "lam",
                                    "sigma_color", "iterations"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [1.0, 0.0, 2, 200, 1.0, 8000.0, 0.25, 3]
    x = torch.zeros(1, 3, 64, 128)
    for name in ("cmfsm", "cmfsm_sub_8"):
        net = ecm_amd.get_model(name)
        for kw, what in (({"head": 3}, "head"), ({"threshold": -1.0}, "threshold"), ({"rel": INF}, "rel"),
                         ({"speckle_size": -1}, "max_size"), ({"speckle_diff": NAN}, "max_diff"), ({"lam": 0.0}, "lam"),
                         ({"lam": NAN}, "lam"), ({"sigma_color": -1.0}, "sigma_color"), ({"iterations": 0}, "iterations"),
                         ({"iterations": 9}, "iterations"), ({"iterations": True}, "iterations")):
            with pytest.raises(ValueError, match=what):
                net.smooth(x, x, **kw)
        with pytest.raises(RuntimeError):
            net.smooth(x, x)
        with pytest.raises(RuntimeError):
            net.smooth(x, x, speckle_size=None)
    assert all(hasattr(cls, "smooth") for cls in models._MODELS.values())
    # the methods that were there keep their parameter lists
    assert list(inspect.signature(models._ECMNet.cross_check).parameters) == ["self", "left", "right", "threshold", "rel", "head"]
