"""The modal disparity of the heads, the part that needs no GPU: a torch restatement of the definitions --
`modal_t` below, any dtype and device, the reference of tests/test_hip_head_mode.py -- checked in fp64 against closed forms and
against the moments of tests/test_head_stats_cpu.py; the ABI additions; predict(mode_radius=...)'s refusals, all of which come
before any device work.

Definitions, for the distribution p over L levels whose mean a head returns (section 15; the levels u pixels apart, u = 1 for
the volume and trilinear heads, u = s for the eight-neighbour head) and a window radius r = radius / u in levels:
index = u D*, D* = argmax p with the lowest D winning an exact tie; W = {D : |D - D*| <= r, 0 <= D < L};
mass = sum_W p, clamped to <= 1; mode = u (D* + sum_W p (D - D*) / sum_W p), centred on D*."""
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

from test_abi_types import declared
from oracle.weights import seeded
from test_head_stats_cpu import cumulative, eight_mixture, moments, one_hot_w9, volume_logits_t

NEW_ENTRIES = ("ecm_aggregate9_mode_fwd", "ecm_volume_mapping_mode_fwd", "ecm_trilinear_softargmin_mode_fwd")


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def modal_t(p, r, index=None, dim=2):
    """(index, mode, mass) in LEVELS of distributions p along `dim`, window radius r levels.  With `index` (integer levels, p's
    shape without `dim`) the window is taken about it and no argmax is computed."""
    L = p.shape[dim]
    if index is None:
        index = p.argmax(dim)                                        # the first maximal value: the lowest level wins a tie
    shape = [1] * p.dim()
    shape[dim] = L
    off = torch.arange(L, device=p.device).view(shape) - index.unsqueeze(dim)
    pw = p * (off.abs() <= r).to(p.dtype)
    sw = pw.sum(dim)
    return index, index.to(p.dtype) + (pw * off.to(p.dtype)).sum(dim) / sw, sw.clamp(max=1)


def eight_p(c, w9, s):
    """The HR pixels' mixtures [NH,B,D',H,W] (levels s pixels apart)."""
    return eight_mixture(c, w9, s)[0]


def volume_p(c, m5, mt3, s):
    return F.softmax(torch.stack([volume_logits_t(L, m5, mt3, s) for L in cumulative(c)], 0), 2)


def trilinear_logits_t(c, Do, H, W):
    """The trilinear head's logits (the first line of test_head_stats_cpu.trilinear_t3): [NH,B,Do,H,W]."""
    return torch.stack([F.interpolate(L.unsqueeze(1), [Do, H, W], mode="trilinear", align_corners=False).squeeze(1)
                        for L in cumulative(c)], 0)


def trilinear_p(c, Do, H, W):
    return F.softmax(trilinear_logits_t(c, Do, H, W), 2)


def two_peaks(L=64, d1=10, d2=30, h1=0.45, h2=0.40):
    p = torch.full((1, 1, L, 1, 1), (1 - h1 - h2) / (L - 2), dtype=torch.float64)
    p[:, :, d1], p[:, :, d2] = h1, h2
    return p


# ---- closed forms and identities, fp64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,r", [(1, 0), (5, 0), (12, 3), (48, 47), (192, 8)])
def test_uniform(L, r):
    index, mode, mass = modal_t(torch.full((2, 1, L, 2, 3), 1 / L, dtype=torch.float64), r)
    assert index.dtype == torch.int64 and bool((index == 0).all())                       # the lowest level wins the tie
    n = min(r, L - 1) + 1                                                                # levels 0..r of the window lie in range
    assert torch.allclose(mass, torch.full_like(mass, n / L), rtol=1e-13)
    assert torch.allclose(mode, torch.full_like(mode, (n - 1) / 2), rtol=0, atol=1e-13)
    if r <= L - 1:
        assert abs(float(mass[0, 0, 0, 0]) - (r + 1) / L) < 1e-13 and abs(float(mode[0, 0, 0, 0]) - r / 2) < 1e-13


def _random_p(name="hm.cpu.p", L=12):
    return F.softmax(seeded(name, 3, 2, L, 4, 5, scale=2.0).double(), 2)


def test_radius_zero_is_the_peak():
    p = _random_p()
    index, mode, mass = modal_t(p, 0)
    _, _, peak, _ = moments(p, 2)
    assert torch.equal(mode, index.double()) and torch.equal(mass, peak)
    assert torch.equal(index, p.argmax(2))


@pytest.mark.parametrize("r", [11, 12, 500])
def test_full_range_is_the_mean(r):
    p = _random_p()
    _, mode, mass = modal_t(p, r)
    mu, _, _, _ = moments(p, 2)
    assert torch.allclose(mode, mu, rtol=0, atol=1e-13) and torch.allclose(mass, torch.ones_like(mass), rtol=0, atol=1e-14)
    assert bool((mass <= 1).all())


def test_two_peaks_the_mode_stays_on_the_higher_one():
    p = two_peaks()
    mu = float(moments(p, 2)[0])
    assert 10 + 2 < mu < 30 - 2                                      # the mean: a depth between the peaks where nothing is
    for r in (0, 1, 2, 8):
        index, mode, mass = modal_t(p, r)
        assert int(index) == 10 and abs(float(mode) - 10) <= r and 0.45 <= float(mass) < 0.45 + 2 * r * 0.15 / 62 + 1e-15
    index, mode, _ = modal_t(p, 2, index=torch.full((1, 1, 1, 1), 30))       # a given index: the window is about it, no argmax
    assert int(index) == 30 and abs(float(mode) - 30) <= 2


def test_lowest_index_wins_an_exact_tie():
    p = torch.zeros(1, 1, 9, 1, 1, dtype=torch.float64)
    p[:, :, 2], p[:, :, 6], p[:, :, 7] = 0.3, 0.3, 0.3
    p[:, :, 0] = 0.1
    index, mode, mass = modal_t(p, 1)
    assert int(index) == 2 and float(mass) == 0.3 and float(mode) == 2.0
    index, mode, mass = modal_t(p, 2)
    assert int(index) == 2 and abs(float(mass) - 0.4) < 1e-15 and abs(float(mode) - (2 - 2 * 0.1 / 0.4)) < 1e-15


def test_window_is_cut_at_the_ends_of_the_range():
    p = torch.tensor([0.5, 0.2, 0.2, 0.1], dtype=torch.float64).view(1, 1, 4, 1, 1)
    _, mode, mass = modal_t(p, 2)                                    # levels -2, -1 do not exist
    assert abs(float(mass) - 0.9) < 1e-15 and abs(float(mode) - (0.2 + 0.4) / 0.9) < 1e-15


def test_any_dtype_and_dim():
    p = _random_p()
    a, b = modal_t(p, 2), modal_t(p.movedim(2, -1).contiguous(), 2, dim=-1)
    assert torch.equal(a[0], b[0]) and all(torch.allclose(x, y, rtol=0, atol=1e-14) for x, y in zip(a[1:], b[1:]))   # another order of summation
    lo = modal_t(p.float(), 2)
    assert lo[1].dtype == torch.float32 and torch.equal(lo[0], a[0]) and torch.allclose(lo[1].double(), a[1], atol=1e-5)


def test_the_three_families_give_distributions():
    """eight_p / volume_p / trilinear_p are the distributions of section 15: their full-range mode is the heads' own mean."""
    NH, B, D, h, w, s = 2, 2, 5, 3, 5, 4
    c = seeded("hm.cpu.c", NH, B, D, h, w, scale=1.5).double()
    w9 = torch.softmax(seeded("hm.cpu.w9", B, 9, h * s, w * s), 1).double()
    m5, mt3 = seeded("hm.cpu.m5", B, 5, h * s, w * s, scale=0.5).double(), seeded("hm.cpu.mt3", B, 3, h * s, w * s, scale=0.5).double()
    for p, L in ((eight_p(c, w9, s), D), (volume_p(c, m5, mt3, s), D * s), (trilinear_p(c, 12, 7, 11), 12)):
        assert p.shape[2] == L and torch.allclose(p.sum(2), torch.ones_like(p.sum(2)), rtol=0, atol=1e-13)
        _, mode, mass = modal_t(p, L - 1)
        assert torch.allclose(mode, moments(p, 2)[0], rtol=0, atol=1e-12) and bool((mass > 1 - 1e-13).all())
    # one-hot centre weights: the eight mixture is the cell's own distribution
    p = eight_p(c, one_hot_w9(B, h * s, w * s), s)
    assert torch.equal(p, F.softmax(cumulative(c), 2).repeat_interleave(s, -1).repeat_interleave(s, -2))


# ---- ABI and wiring ------------------------------------------------------------------------------------------------------------------
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
    assert lib_mod.query("ecm_abi_version") >= 9
    P = lib_mod.PROTOTYPES                                            # the parents' operands, `modal` for disp + stats, plus radius
    assert len(P["ecm_aggregate9_mode_fwd"][1]) == len(P["ecm_aggregate9_stats_fwd"][1]) + 1
    assert len(P["ecm_volume_mapping_mode_fwd"][1]) == len(P["ecm_volume_mapping_stats_fwd"][1])
    assert len(P["ecm_trilinear_softargmin_mode_fwd"][1]) == len(P["ecm_trilinear_softargmin_stats_fwd"][1])


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    lib = lib_mod.load()
    assert lib.ecm_aggregate9_mode_fwd(None, 1, None, None, None, 1, 1, 1, 1, 1, 4, 0, None) == -1
    assert lib.ecm_volume_mapping_mode_fwd(None, 1, None, None, None, 1, 1, 1, 1, 1, 4, 0, None) == -1
    assert lib.ecm_trilinear_softargmin_mode_fwd(None, 1, None, 1, 1, 1, 1, 1, 4, 4, 4, 0, None) == -1


def test_ops_and_namedtuples_are_wired():
    import ecm_amd
    from ecm_amd import models
    for name in ("ecm_aggregate9_mode", "volume_mapping_mode", "trilinear_softargmin_mode"):
        assert callable(getattr(ecm_amd.ops, name)), name
    assert models.Prediction._fields == ("disparity", "std", "peak", "entropy")          # predict() returns what it did
    assert models.ModalPrediction._fields == models.Prediction._fields + ("mode", "mass", "index")
    sig = inspect.signature(models._ECMNet.predict)
    assert list(sig.parameters) == ["self", "left", "right", "heads", "mode_radius"] and sig.parameters["mode_radius"].default is None


# ---- predict(mode_radius=...) refuses before any device work: all of this runs on CPU tensors -------------------------------------------
@pytest.mark.parametrize("name,why", [("cmfsm_sub_8", "do not sum to one"), ("cmf", "refinement decoder")])
def test_predict_refuses_heads_without_a_distribution(name, why):
    import ecm_amd
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(NotImplementedError, match=why):
        ecm_amd.get_model(name).predict(x, x, mode_radius=8)


@pytest.mark.parametrize("arch,bad", [("cmfsm", -4), ("cmfsm", 2.0), ("cmfsm", 6), ("cmfsm", True), ("cm_sub_8", -1), ("cm_sub_8", 1.5),
                                      ("bilinear_cmf", "8")])
def test_predict_checks_the_radius_on_the_cpu(arch, bad):
    import ecm_amd
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(ValueError, match="radius"):
        ecm_amd.get_model(arch).predict(x, x, mode_radius=bad)


def test_op_level_radius_check():
    import ecm_amd
    chk = ecm_amd.ops.check_mode_radius
    assert chk(0) == 0 and chk(8, 4) == 8 and chk(7) == 7
    for bad, scale in ((-1, 1), (0.5, 1), (6, 4), (None, 1)):
        with pytest.raises(ValueError, match="radius"):
            chk(bad, scale)
