"""The left-right consistency check on the MI355X: ops.lr_check and _ECMNet.cross_check against
lr_check_t, the torch restatement of tests/test_lr_check_cpu.py, in fp64 on the CPU.

Exact cases.  Every disparity is a multiple of 1/8 of small magnitude, so x - d, t and the interpolation are exact in fp32
whatever the contraction, and all four outputs (src included) must equal the fp64 restatement bit for bit.  Row n of a case
(n = b H + y) holds the constant K_ROWS[n % 5] on both sides -- positive (the left border is out of view), negative (the right
border is), zero, 16 (where rel = 0.05 takes over from a threshold of 0.5) -- the right plane wiggles by 1/4 px in every other
block of 16 columns (so the interpolation has something to mix), consistent columns carry errors of 0, 1/8, 1/2, 3/4 and 1 px
(1/2 and 1 are the two thresholds: `<=` must pass them), and a validity pattern says which columns stay consistent; the others
are pushed 3 px up or down, which makes them kinds 1, 2 and 3.  The patterns: all; none; one consistent column at 0, W-1, 63,
64; alternating; and, at every boundary p of the kernel's scan that lies inside the row, an inconsistent run [p-2, p+2), a
lone consistent column at p-1 and a lone one at p.  The boundaries are read from csrc/lr_check.hip: CHUNK = 4 (a thread's
chunk: p = 4, 8), WAVE * CHUNK = 256 (a wave: p = 256, 512, 768), SWEEP = THREADS * CHUNK = 1024 (a sweep of the workgroup:
p = 1024, 2048, 3072), to which the tests add 63/64/65 (a wave of columns).  Unperturbed consistent columns of a row are equal,
so most fills are ties dl[Lx] == dl[Rx] (src must be Lx); the columns with an error of 1/8 ... 1 differ, so the others are not.
[1,577,7] has more rows than the launch has workgroups (GRID = 512).

Float cases (test_lr_check_cpu.float_case; its borderline share is asserted there): the project's yardstick
max|error - error64| <= 4 e32 + 2e-7 max|error64| with e32 the error of the fp32 restatement on the device; infinities and
kinds as fp64 has them except at pixels within that bound of a decision (at most 1 % of a case); filled and src exactly the
scans of the kernel's own kind plane.  Prints `LRRATIO <case> <ratio>`; section 17 records the worst."""
import pytest
import torch

from test_hip_guard_bands import POISON, guarded
from test_lr_check_cpu import FLOAT_CASES, fill_t, float_case, kernel_constants, lr_check_t

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, FLOOR, SHARE = 4, 2e-7, 0.01
KC = kernel_constants()
K_ROWS = (1.375, -1.375, 0.0, 16.0, 2.5)


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def boundaries(W):
    ps = {KC["CHUNK"], 2 * KC["CHUNK"], 64}
    ps |= set(range(KC["WAVE"] * KC["CHUNK"], W, KC["WAVE"] * KC["CHUNK"])) | set(range(KC["SWEEP"], W, KC["SWEEP"]))
    return sorted(p for p in ps if 2 <= p <= W - 2)


def patterns(W):
    """name -> (bool [W]: the columns that stay consistent, rotation of K_ROWS)."""
    x = torch.arange(W)
    out = {"all": (torch.ones(W, dtype=torch.bool), 0), "none": (torch.zeros(W, dtype=torch.bool), 0), "alternating": (x % 2 == 0, 0)}
    for c, rot in ((0, 1), (W - 1, 0), (63, 0), (64, 1)):
        if 0 <= c < W:
            out[f"single{c}"] = (x == c, rot)
    ps = boundaries(W)
    if ps:
        run = torch.ones(W, dtype=torch.bool)
        for p in ps:
            run[p - 2:p + 2] = False
        out["runs"] = (run, 0)
        out["before"] = ((x.view(-1, 1) == torch.tensor(ps) - 1).any(1), 0)
        out["at"] = ((x.view(-1, 1) == torch.tensor(ps)).any(1), 1)
    return out


def exact_case(shape, keep, rot):
    B, H, W = shape
    x = torch.arange(W)
    k = torch.tensor([K_ROWS[(n + rot) % len(K_ROWS)] for n in range(B * H)], dtype=torch.float64).view(B, H, 1)
    if W == 1:
        k = k * 0
    dr = k + 0.25 * ((x % 2) * ((x // 16) % 2)).double()
    bump = torch.zeros(W, dtype=torch.float64)
    for m, v in ((5, 0.125), (8, 1.0), (9, 0.75), (10, 0.5)):         # x % 32 == 8, 10: the two thresholds, read where dr is flat
        bump[x % 32 == m] = v
    push = torch.where(x % 3 == 0, -3.0, 3.0).double() + 0.125 * (x % 2)
    dl = k + torch.where(keep, bump, push)
    return dl.float().expand(B, H, W).contiguous(), dr.float().expand(B, H, W).contiguous()


def assert_bitwise(ecm, dl, dr, thr, rel, what, want_tie=False):
    for mirrored in (False, True):
        drm = dr.flip(2).contiguous() if mirrored else dr
        ref = lr_check_t(dl.double(), drm.double(), thr, rel, mirrored)
        got = ecm.ops.lr_check(dl.to(DEV), drm.to(DEV), thr, rel, mirrored=mirrored, with_source=True)
        assert got[3].dtype == torch.int32 and all(t.shape == dl.shape for t in got)
        for name, g, r in zip(("error", "kind", "filled", "src"), got, ref):
            g = g.cpu().long() if name == "src" else g.cpu().double()
            bad = (g != r).nonzero()
            assert bad.numel() == 0, f"{what} mirrored={mirrored}: {name} differs at {bad[:4].tolist()}: {g[tuple(bad[0])]} != {r[tuple(bad[0])]}"
        assert not want_tie or bool(((ref[0] == thr) & (ref[1] == 0)).any()), f"{what}: no error equals the threshold"


SHAPES = [(2, 3, 1), (1, 2, 5), (2, 2, 63), (1, 3, 64), (2, 2, 65), (1, 2, 257), (1, 2, 1030), (1, 1, KC["MAX_W"]), (1, 577, 7)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_exact_cases(ecm, shape):
    assert KC["MAX_W"] == ecm.ops.lr_check_max_width() and 577 > KC["GRID"]
    for name, (keep, rot) in patterns(shape[2]).items():
        dl, dr = exact_case(shape, keep, rot)
        for thr in (1.0, 0.5):
            for rel in (0.0, 0.05):
                assert_bitwise(ecm, dl, dr, thr, rel, f"{shape} {name} thr {thr} rel {rel}", want_tie=name == "all" and shape[2] >= 63)
    ecm.ops.check_async_errors()


def test_rel_takes_over_on_the_device(ecm):
    dl, dr = exact_case((1, 5, 257), torch.ones(257, dtype=torch.bool), 0)
    k0 = ecm.ops.lr_check(dl.to(DEV), dr.to(DEV), 0.5, 0.0)[1]
    k5 = ecm.ops.lr_check(dl.to(DEV), dr.to(DEV), 0.5, 0.05)[1]
    col = torch.arange(257, device=DEV) % 32 == 9                      # error 3/4 at d = 16.75: tol 0.5 against 0.8375
    assert bool((k0[0, 3, 32:][col[32:]] == 2).all()) and bool((k5[0, 3, 32:][col[32:]] == 0).all())
    assert torch.equal(k0[0, :3], k5[0, :3])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_inputs(ecm, bad):
    for shape in ((2, 2, 65), (1, 2, 1030)):
        W = shape[2]
        dl, dr = exact_case(shape, torch.ones(W, dtype=torch.bool), 0)
        for c in (0, 7, 63, 64, W - 1):
            dl[0, 0, c] = bad
        for c in (1, 20, 62, W - 2):
            dr[0, 1, c] = bad
        dl[0, 1, 33] = bad
        assert_bitwise(ecm, dl, dr, 1.0, 0.05, f"{shape} planted {bad}")
        got = ecm.ops.lr_check(dl.to(DEV), dr.to(DEV))
        assert bool((got[1][0, 0, [0, 7, 63, 64, W - 1]] == 3).all()) and bool((got[1][0, 1, 33] == 3).all())
        assert bool((got[1][0, 1] == 2).any()) and bool(torch.isfinite(got[2]).all())


# ---- float cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,rel", [(1.0, 0.0), (0.5, 0.05)])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("name,seed,shape", FLOAT_CASES, ids=[c[0] for c in FLOAT_CASES])
def test_float_cases(ecm, name, seed, shape, mirrored, thr, rel):
    dl, dr = float_case(seed, shape)
    if mirrored:
        dr = dr.flip(2).contiguous()
    W = shape[2]
    e64, k64, _, _ = lr_check_t(dl.double(), dr.double(), thr, rel, mirrored)
    dld, drd = dl.to(DEV), dr.to(DEV)
    e32 = lr_check_t(dld, drd, thr, rel, mirrored)[0].cpu().double()
    err, kind, filled, src = ecm.ops.lr_check(dld, drd, thr, rel, mirrored=mirrored, with_source=True)
    fin = torch.isfinite(e64)
    assert bool(torch.isfinite(e32[fin]).all())
    bound = K * float((e32 - e64)[fin].abs().max()) + FLOOR * float(e64[fin].abs().max())
    # the decisions and the pixels that sit within the bound of one
    xr = torch.arange(W, dtype=torch.float64) - dl.double()
    tol = torch.maximum(torch.full_like(e64, thr), rel * dl.double())
    edge = (xr.abs() <= bound) | ((xr - (W - 1)).abs() <= bound)
    aside = edge | (fin & (((e64 - tol).abs() <= bound) | (e64 <= bound)))
    share = float(aside.double().mean())
    e, k = err.cpu().double(), kind.cpu().double()
    assert torch.equal(torch.isinf(e) | edge, ~fin | edge), f"{name}: infinities are not where fp64 has them"
    both = fin & torch.isfinite(e)
    worst = float((e - e64)[both].abs().max())
    ratio = worst / bound
    print(f"LRRATIO {name} {ratio:.3f}   # thr {thr} rel {rel} mirrored {mirrored}: err {worst:.3e}, bound {bound:.3e}, set aside {share:.5f}")
    assert worst <= bound, f"{name}: |hip - fp64| = {worst:.3e} > {bound:.3e} (ratio {ratio:.2f})"
    assert bool((k == k64)[~aside].all()), f"{name}: kind differs from fp64 away from every decision"
    assert share <= SHARE, f"{name}: {share:.3%} of the pixels are within the bound of a decision (cap {SHARE:.0%})"
    want_filled, want_src = fill_t(dld, kind == 0)
    assert torch.equal(filled, want_filled) and torch.equal(src.long(), want_src)
    ecm.ops.check_async_errors()


# ---- the op's contract ---------------------------------------------------------------------------------------------------------------
def test_shapes_strides_and_streams(ecm):
    ops = ecm.ops
    dl, dr = (t.to(DEV) for t in float_case(7, (2, 6, 130)))
    want = ops.lr_check(dl, dr, 1.0, 0.05, with_source=True)
    assert len(want) == 4 and len(ops.lr_check(dl, dr)) == 3 and all(not t.requires_grad for t in want)
    same = lambda got: all(torch.equal(a, b) for a, b in zip(got, want))                     # noqa: E731
    assert same(ops.lr_check(dl.unsqueeze(1), dr.unsqueeze(1), 1.0, 0.05, with_source=True))
    assert same(ops.lr_check(dl.unsqueeze(1), dr, 1.0, 0.05, with_source=True))
    wide_l, wide_r = torch.zeros(2, 6, 260, device=DEV), torch.zeros(2, 130, 6, device=DEV)
    wide_l[:, :, ::2], wide_r[:] = dl, dr.transpose(1, 2)
    nl, nr = wide_l[:, :, ::2], wide_r.transpose(1, 2)
    assert not nl.is_contiguous() and not nr.is_contiguous()
    assert same(ops.lr_check(nl, nr, 1.0, 0.05, with_source=True))
    assert same(ops.lr_check(dl.clone().requires_grad_(), dr, 1.0, 0.05, with_source=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.lr_check(dl, dr, 1.0, 0.05, with_source=True)
    side.synchronize()
    assert same(got)
    with pytest.raises(RuntimeError, match="disp_r"):
        ops.lr_check(dl, dr[:, :, :-1])
    with pytest.raises(RuntimeError, match="fp32"):
        ops.lr_check(dl.double(), dr.double())
    with pytest.raises(ValueError, match="threshold"):
        ops.lr_check(dl, dr, threshold=-1)
    ops.check_async_errors()


def test_guard_bands_and_the_width_refusal(ecm):
    ops = ecm.ops
    for shape in SHAPES:
        dl, dr = (t.to(DEV) for t in exact_case(shape, torch.arange(shape[2]) % 2 == 0, 0))
        with guarded(ecm) as g:
            ops.lr_check(dl, dr, with_source=True)
            g.check(f"lr_check {shape}")
            assert len(g.records) == 2                               # check, src
    wide = torch.zeros(1, 2, ops.lr_check_max_width() + 1, device=DEV)
    with guarded(ecm) as g:
        with pytest.raises(RuntimeError, match="not supported"):
            ops.lr_check(wide, wide, with_source=True)
        g.check("lr_check beyond the maximum width")
        assert len(g.records) == 2
        for raw, off, n in g.records:
            assert bool((raw[off:off + n] == POISON).all()), "a refused call wrote to its outputs"
    ops.check_async_errors()


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _frames(H, W, B=1):
    g = torch.Generator(device=DEV).manual_seed(11)
    return torch.randn(B, 3, H, W, device=DEV, generator=g), torch.randn(B, 3, H, W, device=DEV, generator=g)


@pytest.mark.parametrize("arch", ["cmfsm", "cmfsm_sub_16", "cmf"])
def test_cross_check_256x512(ecm, arch):
    H, W = 256, 512
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model(arch).to(DEV).eval()
    left, right = _frames(H, W)
    with torch.no_grad():
        fwd = model(left, right)[2].reshape(1, 1, H, W)
        fwd_r = model(torch.flip(right, (-1,)), torch.flip(left, (-1,)))[2].reshape(1, 1, H, W)
    cc = model.cross_check(left, right, threshold=1.0, rel=0.05)
    assert type(cc).__name__ == "CrossCheck" and all(f.shape == (1, 1, H, W) and not f.requires_grad for f in cc)
    assert torch.equal(cc.disparity, fwd), f"{arch}: .disparity differs from forward"
    assert torch.equal(cc.disparity_right, torch.flip(fwd_r, (-1,))), f"{arch}: .disparity_right differs from the flipped forward"
    again = ops.lr_check(fwd, fwd_r, 1.0, 0.05, mirrored=True)
    assert all(torch.equal(f[:, 0], a) for f, a in zip(cc[2:], again))
    plain = ops.lr_check(cc.disparity, cc.disparity_right, 1.0, 0.05)     # the un-mirrored plane, un-mirrored
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    x = torch.arange(W, device=DEV).view(1, 1, 1, W)
    border = x < cc.disparity.amin(3, keepdim=True)
    assert bool((cc.kind[border] == 3).all()) and bool(torch.isinf(cc.error[cc.kind == 3]).all())
    assert bool(((cc.kind >= 0) & (cc.kind <= 3) & (cc.kind == cc.kind.round())).all())
    assert torch.equal(cc.filled[cc.kind == 0], cc.disparity[cc.kind == 0])
    other = model.cross_check(left, right, head=0)
    with torch.no_grad():
        assert torch.equal(other.disparity, model(left, right)[0].reshape(1, 1, H, W))
    ops.check_async_errors()


def test_cross_check_in_bf16(ecm):
    H, W = 256, 512
    ops = ecm.ops
    torch.manual_seed(5)
    model = ecm.get_model("cmfsm").to(DEV).eval()
    left, right = _frames(H, W)
    with ops.inference_dtype(torch.bfloat16), ops.frozen_weights(), torch.no_grad():
        fwd16 = model(left, right)[2].reshape(1, 1, H, W)
        cc = model.cross_check(left, right)
    assert torch.equal(cc.disparity, fwd16) and cc.error.dtype == torch.float32
    ok = cc.kind == 0
    assert bool(torch.isfinite(cc.error[ok]).all()) and bool(torch.isfinite(cc.filled[ok]).all()) and bool(torch.isfinite(cc.disparity[ok]).all())
    ops.check_async_errors()
