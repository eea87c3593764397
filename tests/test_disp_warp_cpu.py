"""The temporal carry (include/ecm_temporal.h), the part that needs no GPU: `warp_t` and `fuse_t` below,
torch restatements of the two definitions -- the references of tests/test_hip_disp_warp.py -- checked against closed forms, ties
and special values; then the census of the fourth header (include/ecm_temporal.h against _lib.TEMPORAL_PROTOTYPES, by the helpers
of tests/test_abi_types.py), its refusal contract with the devices hidden (by the machinery of tests/test_abi_refusals.py), and the
refusals of ops.warp_matrix, ops.disparity_warp, ops.disparity_fuse and models.DisparityTracker that come before any device work.

warp_t evaluates [a b c w] = M [x y d 1] in fp64 with separate multiplies and adds in the header's order, packs the key as
bits(dn) * 2^32 + index in an int64 (dn > 0, so its bits stay below 2^31 and the key fits a signed int64) and reduces with
scatter_reduce_("amax"): an integer maximum, as the kernel's.  Attributes follow by gather.  fuse_t is the update in fp64."""
import ctypes as C
import inspect
import json
import os
import subprocess
import sys

import pytest
import torch

import abi_refusal_child as child
from conftest import ROOT
from test_abi_refusals import EINVAL, HIDE, Row, _report, calls_of, classify, classify_query, query_calls
from test_abi_types import INCLUDE, _strip, compare, lib_mod, package_entry_names, parse_header  # noqa: F401  (lib_mod: a fixture)
from test_disp_splat_cpu import splat_t

HEADER = "ecm_temporal.h"
PREFIX = "ecmt_"
ENTRIES = ("ecmt_disparity_fuse_fwd", "ecmt_disparity_warp_fwd", "ecmt_disparity_warp_max_attributes",
           "ecmt_disparity_warp_scratch_bytes")
NAN, INF = float("nan"), float("inf")
FLT_MAX = 3.4028234663852886e38
FOOTPRINTS = ("cover", "nearest")


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def warp_t(d, M, valid=None, attributes=None, min_disp=0.0, max_disp=None, footprint="cover"):
    """(out [B,H,W] fp32, src [B,H,W] int64, attrs_out [B,C,H,W] or None) of d [B,H,W] fp32 and M [4,4] or [B,4,4]."""
    assert d.dtype == torch.float32 and d.dim() == 3 and footprint in FOOTPRINTS
    B, H, W = d.shape
    m = M.to(torch.float64).expand(B, 4, 4)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    dd = d.to(torch.float64)

    def row(r):
        e = lambda c: m[:, r, c].view(B, 1, 1)                                                   # noqa: E731
        return ((e(0) * x + e(1) * y) + e(2) * dd) + e(3)

    w = row(3)
    lo = torch.tensor(min_disp, dtype=torch.float32)
    hi = torch.tensor(FLT_MAX if max_disp is None else max_disp, dtype=torch.float32)
    usable = torch.isfinite(d) & (d > lo) & (d <= hi) & torch.isfinite(w) & (w != 0)
    if valid is not None:
        usable = usable & (valid != 0)
    u, v, dn = row(0) / w, row(1) / w, (row(2) / w).to(torch.float32)
    cand = usable & torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(dn) & (dn > 0) \
        & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    index = torch.arange(H * W).view(1, H, W)
    key = dn.contiguous().view(torch.int32).long() * (1 << 32) + index
    zero = torch.zeros_like(key)
    u, v = torch.where(cand, u, 0.0), torch.where(cand, v, 0.0)
    best = torch.zeros(B, H * W, dtype=torch.int64)

    def land(yy, xx, on):
        best.scatter_reduce_(1, (yy * W + xx).view(B, -1), torch.where(on, key, zero).view(B, -1), "amax")

    if footprint == "cover":
        fu, fv = u.floor(), v.floor()
        x0, y0 = fu.long(), fv.long()
        right, down = cand & (u > fu), cand & (v > fv)
        x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
        land(y0, x0, cand)
        land(y0, x1, right)
        land(y1, x0, down)
        land(y1, x1, right & down)
    else:
        land((v + 0.5).floor().long().clamp(max=H - 1), (u + 0.5).floor().long().clamp(max=W - 1), cand)
    hole = best == 0
    out = torch.where(hole, torch.zeros(()), (best >> 32).to(torch.int32).view(torch.float32))
    src = torch.where(hole, -1, best & 0xFFFFFFFF)
    attrs_out = None
    if attributes is not None:
        Cn = attributes.shape[1]
        got = attributes.flatten(2).gather(2, src.clamp(min=0).unsqueeze(1).expand(-1, Cn, -1))
        attrs_out = torch.where(hole.unsqueeze(1), torch.zeros(()), got).view(B, Cn, H, W)
    return out.view(B, H, W), src.view(B, H, W), attrs_out


BRANCHES = ("neither", "coast", "dropped", "measurement", "gated", "fused")


def fuse_t(disp, var, prev, prev_var, prev_age=None, prev_source=None, gate=3.0, process_noise=0.0, coast=True):
    """(fused, fused_var fp64; age int64; branch int64, an index into BRANCHES; s, the predicted variance; margin, how far the
    gate's two sides are apart relative to the right side, +inf where no gate is evaluated) of fp32 planes, in fp64."""
    f64 = lambda t: t.to(torch.float64)                                                         # noqa: E731
    d, vr, p, pv = f64(disp), f64(var), f64(prev), f64(prev_var)
    g = float(torch.tensor(gate, dtype=torch.float32))
    q = float(torch.tensor(process_noise, dtype=torch.float32))
    pa = torch.zeros(disp.shape, dtype=torch.int64) if prev_age is None else prev_age.long()
    meas = torch.isfinite(d) & (d > 0) & torch.isfinite(vr) & (vr > 0)
    pred = (p > 0) & torch.isfinite(pv) & (pv > 0)
    if prev_source is None:
        s = pv + q
    else:
        r = p / f64(prev_source)
        s = pv * r * r * r * r + q
    e, total = d - p, s + vr
    inside = e * e <= g * g * total
    both = meas & pred
    K = s / total
    z, zi = torch.zeros_like(d), torch.zeros_like(pa)
    branch = torch.where(both, torch.where(inside, 5, 4), torch.where(meas, 3, torch.where(pred, 1 if coast else 2, 0)))
    fused = torch.where(branch == 5, p + K * e, torch.where(branch >= 3, d, torch.where(branch == 1, p, z)))
    fvar = torch.where(branch == 5, (1 - K) * s, torch.where(branch >= 3, vr, torch.where(branch == 1, s, z)))
    age = torch.where(branch == 5, pa + 1, torch.where(branch >= 3, 1, torch.where(branch == 1, pa, zi)))
    margin = torch.where(both, (e * e - g * g * total).abs() / (g * g * total), torch.full_like(d, INF))
    return fused, fvar, age, branch, s, margin


# ---- the cases the GPU test shares ----------------------------------------------------------------------------------------------------
def shear():
    """The Q^-1 T Q of a sideways translation by one baseline: u = x - d, and nothing else changes."""
    M = torch.eye(4, dtype=torch.float64)
    M[0, 2] = -1.0
    return M


def axial(k):
    """The Q^-1 T Q of a translation along the optical axis (principal point at the origin): w = 1 - k d."""
    M = torch.eye(4, dtype=torch.float64)
    M[3, 2] = -k
    return M


def quantised(B, H, W, seed, top=None):
    """Disparities on the 1/64 px grid in [1/64, top] (top below 4096): there (float)x - d is exact in fp32, so that the splat,
    which forms x - d in fp32, and the warp, which forms it in fp64, decide on the same number."""
    top = min(W - 1, 4095) if top is None else top
    n = torch.randint(1, max(int(top * 64), 2), (B, H, W), generator=torch.Generator().manual_seed(seed))
    return n.to(torch.float32) / 64.0


def rotation(rx, ry, rz):
    """A rotation matrix from three small angles (radians), fp64: Rz Ry Rx."""
    t = lambda v: torch.tensor(v, dtype=torch.float64)                                           # noqa: E731
    cx, sx, cy, sy, cz, sz = (f(t(a)) for a in (rx, ry, rz) for f in (torch.cos, torch.sin))
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return Rz @ Ry @ Rx


def rigid(rx, ry, rz, tx, ty, tz):
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = rotation(rx, ry, rz)
    T[:3, 3] = torch.tensor([tx, ty, tz], dtype=torch.float64)
    return T


def ecm():
    import ecm_amd
    return ecm_amd


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("footprint", FOOTPRINTS)
def test_the_identity_returns_the_usable_pixels(footprint):
    B, H, W = 2, 5, 9
    g = torch.Generator().manual_seed(1)
    d = 0.5 + 60 * torch.rand(B, H, W, generator=g)
    r = torch.rand(B, H, W, generator=g)
    for k, bad in enumerate((NAN, INF, -INF, 0.0, -0.0, -3.5)):
        d[(r >= 0.05 * k) & (r < 0.05 * (k + 1))] = bad
    valid = torch.rand(B, H, W, generator=g) < 0.8
    index = torch.arange(H * W).view(1, H, W).expand(B, H, W)
    attrs = torch.rand(B, 2, H, W, generator=g)
    out, src, a = warp_t(d, torch.eye(4, dtype=torch.float64), valid, attrs, footprint=footprint)
    usable = torch.isfinite(d) & (d > 0) & valid
    assert 0 < int(usable.sum()) < B * H * W
    assert torch.equal(bits(out), torch.where(usable, bits(d), 0))
    assert torch.equal(src, torch.where(usable, index, -1))
    assert torch.equal(bits(a), torch.where(usable.unsqueeze(1), bits(attrs), 0))


def test_the_shear_is_the_splat():
    """M = I with M[0][2] = -1 under "cover" is disparity_splat's definition on positive disparities: u = x - d, v = y, dn = d; the
    key orders by the disparity's bits, then by y * W + x, which within a row is the splat's order by column.  The splat forms
    x - d in fp32 and the warp in fp64: on the 1/64 px grid below 4096 both are exact, hence the quantised input."""
    for B, H, W, seed in ((2, 3, 70, 3), (1, 2, 300, 4), (1, 4, 17, 5)):
        d = quantised(B, H, W, seed)
        right, col = splat_t(d)
        out, src, _ = warp_t(d, shear())
        assert torch.equal(bits(out), bits(right))
        rows = torch.arange(H).view(1, H, 1) * W
        assert torch.equal(torch.where(src >= 0, src - rows, -1), col)
        assert 0 < int((src < 0).sum()) < B * H * W


def test_a_forward_motion_scales_a_constant_plane_about_the_origin():
    H, W, d0, k = 9, 13, 16.0, 1.0 / 64.0                                 # w = 1 - k d = 0.75: the image magnifies by 4/3
    d = torch.full((1, H, W), d0)
    dn = torch.tensor(d0 / 0.75, dtype=torch.float64).to(torch.float32)
    # nearest: source x lands on floor(x / 0.75 + 0.5) where x / 0.75 <= W-1, i.e. x <= 0.75 (W-1) = 9 (exact: W-1 is a multiple
    # of 4); the landings are 4/3 apart, so no two share a site
    nx, ny = int(0.75 * (W - 1)) + 1, int(0.75 * (H - 1)) + 1
    out, src, _ = warp_t(d, axial(k), footprint="nearest")
    assert int((src < 0).sum()) == H * W - nx * ny
    for ys in range(ny):
        for xs in range(nx):
            yt, xt = int(ys / 0.75 + 0.5), int(xs / 0.75 + 0.5)
            assert src[0, yt, xt] == ys * W + xs
    assert bool((bits(out)[src >= 0] == bits(dn)).all()) and bool((bits(out)[src < 0] == 0).all())
    # cover: a magnification below 2 leaves no hole (consecutive landings are less than two sites apart)
    out, src, _ = warp_t(d, axial(k), footprint="cover")
    assert int((src < 0).sum()) == 0 and bool((bits(out) == bits(dn)).all())
    assert src[0, 0, 0] == 0 and src[0, H - 1, W - 1] == (ny - 1) * W + nx - 1


def test_warp_matrix_closed_forms():
    ops = ecm().ops
    f, b, tz = 700.0, 0.25, 0.1
    T = torch.eye(4, dtype=torch.float64)
    T[2, 3] = -tz                                                          # the camera moves forward: every point comes closer
    M = ops.warp_matrix(ops.q_matrix(f, b, 0.0, 0.0), T)
    assert M.dtype == torch.float64 and M.shape == (4, 4) and not M.is_cuda
    assert float((M - axial(tz / (b * f))).abs().max()) <= 1e-12
    T = torch.eye(4, dtype=torch.float64)
    T[0, 3] = -b                                                           # one baseline sideways: the right camera's view
    Q = ops.q_matrix(f, b, 320.5, 240.25, x0=16, y0=8)
    assert float((ops.warp_matrix(Q, T) - shear()).abs().max()) <= 1e-12
    assert float((ops.warp_matrix(Q, torch.eye(4, dtype=torch.float64)) - torch.eye(4, dtype=torch.float64)).abs().max()) <= 1e-12
    both = ops.warp_matrix(Q, torch.stack([T, torch.eye(4, dtype=torch.float64)]), Q_out=Q)
    assert both.shape == (2, 4, 4) and float((both[0] - shear()).abs().max()) <= 1e-12


def test_warp_matrix_refusals():
    ops = ecm().ops
    Q, I = ops.q_matrix(700.0, 0.25, 3.0, 2.0), torch.eye(4, dtype=torch.float64)
    for bad in (I.float(), torch.eye(3, dtype=torch.float64), I.view(1, 1, 4, 4), "I", None, torch.zeros(0, 4, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="warp_matrix: T"):
            ops.warp_matrix(Q, bad)
        with pytest.raises(ValueError, match="warp_matrix: Q"):
            ops.warp_matrix(bad, I)
    nan = I.clone()
    nan[1, 2] = NAN
    with pytest.raises(ValueError, match="non-finite"):
        ops.warp_matrix(Q, nan)
    with pytest.raises(ValueError, match="singular"):
        ops.warp_matrix(Q, I, Q_out=torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="batch"):
        ops.warp_matrix(torch.stack([Q] * 2), torch.stack([I] * 3))


# ---- ties and special values ----------------------------------------------------------------------------------------------------------
def test_the_larger_index_wins_a_tie_and_the_larger_disparity_wins():
    d = torch.full((1, 1, 16), NAN)
    d[0, 0, 10], d[0, 0, 11] = 3.5, 3.5                                   # 6.5 -> 6, 7 and 7.5 -> 7, 8: column 7 takes source 11
    out, src, _ = warp_t(d, shear())
    assert src[0, 0, 6:9].tolist() == [10, 11, 11] and int((src >= 0).sum()) == 3
    d = torch.tensor([[[NAN, NAN, NAN, 1.0, 2.0, NAN]]])                  # column 2: d = 2 from 4 beats d = 1 from 3
    out, src, _ = warp_t(d, shear())
    assert src[0, 0].tolist() == [-1, -1, 4, -1, -1, -1] and out[0, 0, 2] == 2.0
    d = torch.full((1, 3, 4), NAN)                                         # two rows onto one: M takes y to y / 2 ... rows 0 and 1
    d[0, 0, 1], d[0, 1, 1] = 5.0, 5.0                                      # both land on (1, 0) under nearest with v = 0.25 y
    M = torch.eye(4, dtype=torch.float64)
    M[1, 1] = 0.25
    out, src, _ = warp_t(d, M, footprint="nearest")
    assert src[0, 0, 1] == 1 * 4 + 1 and int((src >= 0).sum()) == 1


def test_special_values_are_decided_as_stated():
    W = 8
    eye = torch.eye(4, dtype=torch.float64)
    for bad in (NAN, INF, -INF, 0.0, -0.0, -1.0):                          # not finite, or d <= min_disp
        d = torch.full((1, 2, W), 2.0)
        d[0, 0, 3] = bad
        out, src, _ = warp_t(d, eye)
        assert src[0, 0, 3] == -1 and bits(out)[0, 0, 3] == 0 and int((src < 0).sum()) == 1
    d = torch.full((1, 1, W), 2.0)
    out, src, _ = warp_t(d, eye, min_disp=2.0)
    assert bool((src == -1).all())
    out, src, _ = warp_t(d, eye, min_disp=1.0, max_disp=2.0)
    assert bool((src >= 0).all())
    valid = torch.ones(1, 1, W, dtype=torch.uint8)
    valid[0, 0, 5] = 0
    assert warp_t(d, eye, valid)[1][0, 0].tolist() == [0, 1, 2, 3, 4, -1, 6, 7]
    M = eye.clone()                                                        # w = d - 2: zero at d = 2, negative below it
    M[3, 2], M[3, 3] = 1.0, -2.0
    d = torch.tensor([[[2.0, 1.0, 3.0, 2.5]]])                            # w = 0: unusable;  w = -1: dn = -1 <= 0;  w = 1: lands on
    out, src, _ = warp_t(d, M, footprint="nearest")                        # (2, 0) with dn = 3;  w = 0.5: u = 6 > W-1: out of view
    assert src[0, 0].tolist() == [-1, -1, 2, -1] and out[0, 0, 2] == 3.0
    for shift, want in ((-2.0, [2, 3, 4, -1, -1]), (2.0, [-1, -1, 0, 1, 2])):   # u exactly 0 and exactly W-1 are inside, on one site
        M = eye.clone()
        M[0, 3] = shift
        for footprint in FOOTPRINTS:
            assert warp_t(torch.full((1, 1, 5), 2.0), M, footprint=footprint)[1][0, 0].tolist() == want
    M = eye.clone()
    M[0, 3] = 2.0 + 2.0 ** -40                                             # just beyond W-1: out
    assert warp_t(torch.full((1, 1, 5), 2.0), M)[1][0, 0].tolist() == [-1, -1, 0, 1, 1]
    M[0, 3] = -2.0 - 2.0 ** -40                                            # just below 0: out
    assert warp_t(torch.full((1, 1, 5), 2.0), M)[1][0, 0].tolist() == [3, 4, 4, -1, -1]


# ---- the fusion -----------------------------------------------------------------------------------------------------------------------
def test_fuse_branches_on_exact_values():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)                                         # noqa: E731
    #            neither  coast  measurement  gated   fused   at the gate    just beyond it
    disp = t(0.0, NAN, 5.0, 20.0, 9.0, 11.0, 11.000001)
    var = t(1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 3.0)
    prev = t(0.0, 8.0, 0.0, 8.0, 8.0, 8.0, 8.0)
    pvar = t(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    page = torch.tensor([7, 7, 7, 7, 7, 7, 7], dtype=torch.int32)
    # s = 1, s + var = 4, gate = 1.5: e^2 <= 9, equality at e = 3; K = 1/4
    fused, fvar, age, branch, s, _ = fuse_t(disp, var, prev, pvar, page, None, gate=1.5)
    assert [BRANCHES[b] for b in branch.tolist()] == ["neither", "coast", "measurement", "gated", "fused", "fused", "gated"]
    assert fused.tolist() == [0.0, 8.0, 5.0, 20.0, 8.25, 8.75, float(disp[6])]
    assert fvar.tolist() == [0.0, 1.0, 2.0, 3.0, 0.75, 0.75, 3.0] and age.tolist() == [0, 7, 1, 1, 8, 8, 1]
    fused, fvar, age, branch, _, _ = fuse_t(disp, var, prev, pvar, page, None, gate=1.5, coast=False)
    assert BRANCHES[branch[1]] == "dropped" and (fused[1], fvar[1], age[1]) == (0.0, 0.0, 0)
    # process noise and the axial propagation: prev / prev_source = 2, so s = 1 * 16 + 0.5
    fused, fvar, age, branch, s, _ = fuse_t(disp, var, prev, pvar, None, t(*[4.0] * 7), gate=1.5, process_noise=0.5)
    assert s[1:].tolist() == [16.5, 0.5, 16.5, 16.5, 16.5, 16.5] and fvar[1] == 16.5 and age.tolist() == [0, 0, 1, 1, 1, 1, 1]
    # a variance that is zero, negative or not finite is no measurement and no prediction
    for bad in (0.0, -1.0, NAN, INF):
        assert BRANCHES[fuse_t(t(5.0), t(bad), t(8.0), t(1.0))[3][0]] == "coast"
        assert BRANCHES[fuse_t(t(5.0), t(1.0), t(8.0), t(bad))[3][0]] == "measurement"


# ---- the census of the fourth header ----------------------------------------------------------------------------------------------------
def header_prototypes():
    with open(os.path.join(INCLUDE, HEADER)) as f:
        return parse_header(f.read())


def test_tables_still_has_three_rows_and_the_fourth_is_registered():
    lib = ecm()._lib
    assert tuple(lib.TABLES) == ("ecm_hip.h", "ecm_geometry.h", "ecm_rectify.h")
    assert tuple(lib.EXTENSION_TABLES) == (HEADER,) and lib.EXTENSION_TABLES[HEADER] == (lib.TEMPORAL_PROTOTYPES, PREFIX)
    assert lib.EXTENSION_TABLES[HEADER][0] is lib.TEMPORAL_PROTOTYPES
    rows = dict(lib._tables())
    assert all(n in rows for n in ENTRIES) and "ecm_abi_version" in rows and "ecmg_reproject_fwd" in rows


def test_header_table_and_package_literals_name_the_same_entries():
    import re
    lib = ecm()._lib
    parsed = header_prototypes()
    with open(os.path.join(INCLUDE, HEADER)) as f:
        by_text = set(re.findall(rf"\b({PREFIX}[a-z0-9_]+)\s*\(", _strip(f.read())))
    found = package_entry_names(PREFIX + "[a-z0-9_]+", "TEMPORAL_PROTOTYPES")
    assert sorted(parsed) == sorted(by_text) == sorted(lib.TEMPORAL_PROTOTYPES) == sorted(found) == sorted(ENTRIES)
    assert all(n.startswith(PREFIX) for n in parsed)
    assert all(a.startswith("ops.py:") for at in found.values() for a in at), found
    for table, _ in lib.TABLES.values():
        assert not set(table) & set(lib.TEMPORAL_PROTOTYPES)


def test_prototypes_match_the_header_type_by_type():
    table, parsed = ecm()._lib.TEMPORAL_PROTOTYPES, header_prototypes()
    assert compare(parsed, table) == []
    assert all(table[n] == parsed[n] for n in parsed)


def test_library_exports_every_row_and_load_types_it(lib_mod):
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(lib, n)] == [] and lib_mod.missing_symbols() == []
    table = lib_mod.TEMPORAL_PROTOTYPES
    real = dict(table)
    try:
        table[PREFIX + "not_there"] = (C.c_int, [])
        assert lib_mod.missing_symbols() == [PREFIX + "not_there"]
    finally:
        table.clear()
        table.update(real)
    loaded = lib_mod.load()
    for name, (res, args) in table.items():
        assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == args, name
    with pytest.raises(RuntimeError, match="does not export"):
        lib_mod.call(PREFIX + "not_there")
    assert ecm().ops.disparity_warp_max_attributes() == lib_mod.query("ecmt_disparity_warp_max_attributes") == 4
    assert lib_mod.query("ecmt_disparity_warp_scratch_bytes", 3, 40, 70) == 3 * 40 * 70 * 8


# ---- the refusal contract, with the devices hidden --------------------------------------------------------------------------------------
ROWS = [
    Row("ecmt_disparity_warp_fwd",
        "disp:p valid:o M:p m_per_image=~0 attrs:o C=-0 out:p src:o attrs_out:o scratch:p scratch_bytes=Q0 B=1 H=1 W=1 "
        "min_disp=f0 max_disp=f100 footprint=~0 stream:s", queries=[("ecmt_disparity_warp_scratch_bytes", "B H W")],
        inval=[{"C": "ecmt_disparity_warp_max_attributes+1"}, {"C": 1, "attrs": None}, {"C": 1, "attrs_out": None}],
        legal=[{"C": 1}, {"footprint": 1}],
        # "footprint outside {0, 1}, H * W >= 2^31, or B * ceil(H * W / 2048) >= 2^24"
        unsup=[{"footprint": 2}, {"footprint": -1}, {"H": 65536, "W": 32768}, {"B": 65536, "H": 4096, "W": 4096}], header=HEADER),
    Row("ecmt_disparity_fuse_fwd",
        "disp:p var:p prev:p prev_var:p prev_age:o prev_source:o fused:p fused_var:p age:p n=L1 gate=f3 process_noise=f0 coast=~1 "
        "stream:s", header=HEADER),
]
QUERIES = [Row("ecmt_disparity_warp_scratch_bytes", "B=1 H=1 W=1", header=HEADER)]
INT_CONSTS = ("ecmt_disparity_warp_max_attributes",)


@pytest.fixture(scope="module")
def results(lib_mod):
    """{call id: return value} of the rows above from one fresh child that sees no device (tests/abi_refusal_child.py)."""
    parsed = header_prototypes()
    calls = [{"id": f"const|{n}", "fn": n, "res": "i", "args": []} for n in INT_CONSTS]
    for row in ROWS:
        calls += calls_of(row, lambda q: parsed[q][1])
    for row in QUERIES:
        calls += query_calls(row)
    assert len({c["id"] for c in calls}) == len(calls)
    env = dict(os.environ)
    env.update(HIDE)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__)], input=json.dumps({"lib": lib_mod.LIB_PATH, "calls": calls}),
                       capture_output=True, text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    seen = next((ln.split()[1] for ln in lines if ln.startswith("DEVICES ")), None)
    assert seen is not None and seen.isdigit(), f"the child did not report a device count (exit {r.returncode}): {r.stderr[-2000:]}"
    if seen != "0":
        pytest.skip(f"the child sees {seen} device(s) although {sorted(HIDE)} hide them: no ABI call was made")
    got = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("R ")}
    if "DONE" not in lines:
        nxt = next((c["id"] for c in calls if c["id"] not in got), None)
        pytest.fail(f"the child ended with status {r.returncode} in call {nxt}: {r.stderr[-2000:]}")
    return got


def test_every_entry_of_the_fourth_header_has_a_row():
    parsed = header_prototypes()
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    assert sorted(ent) == sorted(r.name for r in ROWS) and sorted(qry) == sorted(r.name for r in QUERIES)
    for r in ROWS + QUERIES:
        assert r.types == (ent.get(r.name) or qry[r.name]), r.name
    assert sorted(set(parsed) - set(ent) - set(qry)) == sorted(INT_CONSTS)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    row = next(r for r in ROWS if r.name == name)
    bad = classify(row, results)
    assert not bad, "\n" + _report(bad)
    assert results[f"{name}|accepted"] > 0                                 # the pointers are never dereferenced: no device, no crash


def test_size_query_is_zero_for_sizes_it_cannot_serve(results):
    row = QUERIES[0]
    bad = classify_query(row, results)
    assert not bad, "\n" + _report(bad)
    answers = {k: v for k, v in results.items() if "|query0" in k or k.startswith(row.name + "|")}   # every call of the query
    assert len(answers) > 10 and all(v >= 0 for v in answers.values()), answers
    assert results["ecmt_disparity_warp_fwd|query0@H=65536,W=32768"] == 0


def test_further_refusals_of_the_two_entries(lib_mod):
    """What the rows cannot express: floats, and an output that is an input.  Every call returns before any HIP call."""
    lib = lib_mod.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(12)]                    # never dereferenced
    warp = lambda **kw: lib.ecmt_disparity_warp_fwd(*[kw.get(k, v) for k, v in (                 # noqa: E731
        ("disp", p[0]), ("valid", p[1]), ("M", p[2]), ("per", 0), ("attrs", p[3]), ("C", 1), ("out", p[4]), ("src", p[5]),
        ("attrs_out", p[6]), ("scratch", p[7]), ("bytes", 8), ("B", 1), ("H", 1), ("W", 1), ("lo", 0.0), ("hi", 100.0), ("fp", 0),
        ("stream", None))])
    for kw in ({"out": p[0]}, {"src": p[0]}, {"attrs_out": p[0]}, {"scratch": p[0]}, {"out": p[3]}, {"out": p[2]}, {"src": p[1]},
               {"lo": NAN}, {"lo": INF}, {"hi": NAN}, {"lo": 2.0, "hi": 1.0}):
        assert warp(**kw) == EINVAL, kw
    assert warp(bytes=7) == -3 and warp(B=2, bytes=15) == -3
    fuse = lambda gate, noise: lib.ecmt_disparity_fuse_fwd(*p[:9], 1, gate, noise, 1, None)      # noqa: E731
    for gate, noise in ((-1.0, 0.0), (NAN, 0.0), (INF, 0.0), (3.0, -1.0), (3.0, NAN), (3.0, INF)):
        assert fuse(gate, noise) == EINVAL, (gate, noise)


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
class OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the shape and dtype contract is checked before anything is launched."""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


def test_op_signatures():
    ops = ecm().ops
    sig = inspect.signature(ops.disparity_warp)
    assert list(sig.parameters) == ["disp", "M", "valid", "attributes", "min_disp", "max_disp", "footprint", "with_source"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, 0.0, None, "cover", False]
    sig = inspect.signature(ops.disparity_fuse)
    assert list(sig.parameters) == ["disp", "var", "prev", "prev_var", "prev_age", "prev_source", "gate", "process_noise", "coast"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [None, None, 3.0, 0.0, True]
    assert list(inspect.signature(ops.warp_matrix).parameters) == ["Q", "T", "Q_out"]
    assert ops.WARP_FOOTPRINTS == FOOTPRINTS


def test_warp_refusals():
    ops = ecm().ops
    eye = torch.eye(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_warp(torch.zeros(1, 4, 8), eye)
    for kw, match in (({"footprint": "bilinear"}, "footprint"), ({"footprint": 0}, "footprint"), ({"min_disp": NAN}, "min_disp"),
                      ({"min_disp": 2.0, "max_disp": 1.0}, "max_disp"), ({"attributes": fake(1, 5, 4, 8)}, "attribute")):
        with pytest.raises(ValueError, match=match):
            ops.disparity_warp(fake(1, 4, 8), eye, **kw)
    for bad in (eye.float(), torch.eye(3, dtype=torch.float64), "M", torch.full((4, 4), NAN, dtype=torch.float64)):
        with pytest.raises(ValueError, match="disparity_warp: M"):
            ops.disparity_warp(fake(1, 4, 8), bad)
    with pytest.raises(ValueError, match="one matrix, or one per image"):
        ops.disparity_warp(fake(2, 4, 8), torch.stack([eye] * 3))
    for bad in (fake(4, 8), fake(1, 2, 4, 8), fake(1, 0, 8)):
        with pytest.raises(RuntimeError, match="disparity_warp"):
            ops.disparity_warp(bad, eye)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.disparity_warp(fake(1, 4, 8, dtype=torch.float64), eye)
    with pytest.raises(RuntimeError, match="valid"):
        ops.disparity_warp(fake(1, 4, 8), eye, valid=fake(1, 4, 8))
    with pytest.raises(RuntimeError, match="attributes"):
        ops.disparity_warp(fake(1, 4, 8), eye, attributes=fake(1, 2, 4, 9))
    assert ops.check_warp_parameters(eye, 1, None, 4, "nearest") == (1.0, FLT_MAX, 1)


def test_fuse_refusals():
    ops = ecm().ops
    z = fake(1, 4, 8)
    for kw, match in (({"gate": -1.0}, "gate"), ({"gate": NAN}, "gate"), ({"process_noise": -0.5}, "process_noise"),
                      ({"gate": True}, "gate"), ({"coast": 1}, "coast")):
        with pytest.raises(ValueError, match=match):
            ops.disparity_fuse(z, z, z, z, **kw)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_fuse(*[torch.zeros(1, 4, 8)] * 4)
    with pytest.raises(RuntimeError, match="prev_var"):
        ops.disparity_fuse(z, z, z, fake(1, 4, 9))
    with pytest.raises(RuntimeError, match="prev_age"):
        ops.disparity_fuse(z, z, z, z, prev_age=z)
    with pytest.raises(RuntimeError, match="var is"):
        ops.disparity_fuse(z, fake(1, 4, 8, dtype=torch.float64), z, z)


def test_tracker_refusals():
    e = ecm()
    models, ops = e.models, e.ops
    net, Q = e.get_model("cmfsm"), ops.q_matrix(700.0, 0.25, 64.0, 32.0)
    sig = inspect.signature(models.DisparityTracker.__init__)
    assert list(sig.parameters) == ["self", "model", "Q", "head", "gate", "process_noise", "sigma0", "footprint", "coast"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [2, 3.0, 0.01, 1.0, "cover", True]
    assert models.Tracked._fields == ("disparity", "std", "warped", "fused", "variance", "age")
    for kw, match in (({"head": 3}, "head"), ({"head": True}, "head"), ({"gate": -1}, "gate"), ({"process_noise": NAN}, "process_noise"),
                      ({"sigma0": 0.0}, "sigma0"), ({"footprint": "both"}, "footprint"), ({"coast": None}, "coast")):
        with pytest.raises(ValueError, match=match):
            models.DisparityTracker(net, Q, **kw)
    with pytest.raises(ValueError, match="model"):
        models.DisparityTracker(torch.nn.Identity(), Q)
    for bad in (Q.float(), torch.zeros(4, 4, dtype=torch.float64), torch.eye(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="warp_matrix"):
            models.DisparityTracker(net, bad)
    tracker = models.DisparityTracker(net, Q)
    assert not isinstance(tracker, torch.nn.Module) and not hasattr(tracker, "parameters")
    x = torch.zeros(1, 3, 64, 128)                                         # CPU tensors: a forward on them raises RuntimeError
    for bad in (torch.eye(4), torch.eye(3, dtype=torch.float64), torch.full((4, 4), INF, dtype=torch.float64)):
        with pytest.raises(ValueError, match="warp_matrix: T"):
            tracker(x, x, motion=bad)
    with pytest.raises(RuntimeError):
        tracker(x, x)
    tracker.reset()
    assert tracker._state is None
