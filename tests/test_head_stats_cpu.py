"""Per-pixel uncertainty of the disparity heads, the part that needs no GPU: the ABI additions, a torch
restatement of the three definitions for each head family -- `eight_t`, `volume_t`, `trilinear_t3` below, any dtype and device,
the reference of tests/test_hip_head_stats.py -- checked in fp64 against closed forms and against the oracle, and predict()'s
refusals.

Definitions, for the distribution p(D) whose mean a head returns: std = sqrt(sum p (D - mu)^2) about p's own mean (written
centred, never sum p D^2 - mu^2), peak = max p, entropy = -sum p ln p in nats with 0 ln 0 = 0.  volume / trilinear: p is the
softmax over the fused full-resolution logits.  eight: p is the mixture sum_n w9[n] p_n / sum_n w9[n] of the low-resolution
softmaxes of the neighbours ecm_aggregate9 does not skip, and std is in full-resolution pixels (s times the mixture's)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import oracle.ecm_oracle as O
from test_abi_types import declared
from oracle.weights import seeded
from test_hip_variants_fullsize import soft_argmin_t, volume_mapping_t

NEW_ENTRIES = ("ecm_softargmin_heads_lse_fwd", "ecm_aggregate9_stats_fwd", "ecm_volume_mapping_stats_fwd",
               "ecm_trilinear_softargmin_stats_fwd")
NBR9 = tuple((dy, dx) for dy, dx, _ in O.EIGHT_NEIGHBOURS)


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def moments(p, dim):
    """(mean, std, peak, entropy) of distributions p along `dim` over the indices 0..D-1."""
    D = p.shape[dim]
    shape = [1] * p.dim()
    shape[dim] = D
    idx = torch.arange(D, device=p.device, dtype=p.dtype).view(shape)
    mu = (p * idx).sum(dim, keepdim=True)
    var = (p * (idx - mu) ** 2).sum(dim)
    return mu.squeeze(dim), var.sqrt(), p.amax(dim), -torch.xlogy(p, p).sum(dim)


def cumulative(c):
    """Head k's logits c_0 + ... + c_k, summed in that order: c [NH,...] -> [NH,...]."""
    out, acc = [], None
    for k in range(c.shape[0]):
        acc = c[k] if acc is None else acc + c[k]
        out.append(acc)
    return torch.stack(out, 0)


def logits_stats(v):
    """v [NH,B,D,H,W] full-resolution logits -> (disp, std, peak, entropy), each [NH,B,H,W]."""
    return moments(F.softmax(v, 2), 2)


def valid9(h, w, s, device):
    """[9,H,W]: 1 where plane n's neighbour cell lies in the image (what aggregate9_fwd does not skip)."""
    cy = torch.arange(h * s, device=device).view(-1, 1) // s
    cx = torch.arange(w * s, device=device).view(1, -1) // s
    return torch.stack([((cy + dy >= 0) & (cy + dy < h) & (cx + dx >= 0) & (cx + dx < w)) for dy, dx in NBR9], 0)


def eight_mixture(c, w9, s):
    """c [NH,B,D',h,w] raw classifier outputs, w9 [B,9,H,W] -> (p [NH,B,D',H,W] the HR pixels' mixtures, wsum [B,H,W] the
    sum of the valid weights, p_lr [NH,B,D',h,w], a [B,9,H,W] the normalised valid weights)."""
    NH, B, D, h, w = c.shape
    p_lr = F.softmax(cumulative(c), 2)
    wv = w9 * valid9(h, w, s, c.device).to(c.dtype)
    wsum = wv.sum(1)
    a = wv / wsum.unsqueeze(1)
    pp = F.pad(p_lr, (1, 1, 1, 1))
    p = 0
    for n, (dy, dx) in enumerate(NBR9):
        nb = pp[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w].repeat_interleave(s, -1).repeat_interleave(s, -2)
        p = p + nb * a[:, n].view(1, B, 1, h * s, w * s)
    return p, wsum, p_lr, a


def eight_t(c, w9, s):
    """(disp, std, peak, entropy) of the eight-neighbour head, each [NH,B,H,W]; disp = s * wsum * mixture mean."""
    p, wsum, _, _ = eight_mixture(c, w9, s)
    mu, std, peak, ent = moments(p, 2)
    return s * wsum.unsqueeze(0) * mu, s * std, peak, ent


def volume_logits_t(cost_lr, m5, mt3, s):
    """The fused logits of cmfsm_sub_16.py:767-798 on [B,Dl,h,w] accumulated logits -> [B,Dl*s,H,W] (the body of
    tests/test_hip_variants_fullsize.volume_mapping_t up to its softmax; test_volume_logits_are_the_established_closed_form)."""
    B, Dl, h, w = cost_lr.shape
    H, W, D = h * s, w * s, Dl * s
    up = cost_lr.repeat_interleave(s, -1).repeat_interleave(s, -2)
    fused = up * m5[:, 0:1]
    for n, (dy, dx) in enumerate(((0, 0), (0, 1), (0, -1), (-1, 0), (1, 0))):
        if n == 0:
            continue
        sh = torch.roll(up, shifts=(-dy * s, -dx * s), dims=(-2, -1))
        ok = torch.ones(1, 1, H, W, device=up.device, dtype=up.dtype)
        if dy < 0: ok[:, :, :s] = 0
        if dy > 0: ok[:, :, H - s:] = 0
        if dx < 0: ok[..., :s] = 0
        if dx > 0: ok[..., W - s:] = 0
        fused = fused + sh * ok * m5[:, n:n + 1]
    fused = fused.repeat_interleave(s, 1)
    X = torch.arange(W, device=up.device).view(1, 1, 1, W)
    Dv = torch.arange(D, device=up.device).view(1, D, 1, 1)
    idx = (X - Dv).expand(B, D, H, W)
    inside = idx >= 0

    def target(pl):
        return torch.where(inside, torch.gather(mt3[:, pl:pl + 1].expand(B, D, H, W), 3, idx.clamp(min=0)),
                           torch.ones((), device=up.device, dtype=up.dtype))
    out = fused * target(0)
    out = out + F.pad(fused[:, s:] * target(2)[:, :-s], (0, 0, 0, 0, 0, s))
    out = out + F.pad(fused[:, :-s] * target(1)[:, s:], (0, 0, 0, 0, s, 0))
    return out


def volume_t(c, m5, mt3, s):
    return logits_stats(torch.stack([volume_logits_t(L, m5, mt3, s) for L in cumulative(c)], 0))


def trilinear_t3(c, Do, H, W):
    up = [F.interpolate(L.unsqueeze(1), [Do, H, W], mode="trilinear", align_corners=False).squeeze(1) for L in cumulative(c)]
    return logits_stats(torch.stack(up, 0))


def spikes(D, at, height=60.0, shape=(1, 1, 1)):
    """[NH=1,B,D,h,w] fp64 logits: `height` at the indices `at`, 0 elsewhere."""
    v = torch.zeros(1, shape[0], D, shape[1], shape[2], dtype=torch.float64)
    for d in at:
        v[:, :, d] = height
    return v


def one_hot_w9(B, H, W, n=0, dtype=torch.float64):
    w9 = torch.zeros(B, 9, H, W, dtype=dtype)
    w9[:, n] = 1
    return w9


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
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
    assert lib_mod.query("ecm_abi_version") >= 8
    # arguments of the parents plus the new buffers
    P = lib_mod.PROTOTYPES
    assert len(P["ecm_softargmin_heads_lse_fwd"][1]) == len(P["ecm_softargmin_heads_fwd"][1]) + 1
    assert len(P["ecm_volume_mapping_stats_fwd"][1]) == len(P["ecm_volume_mapping_fwd"][1]) + 1
    assert len(P["ecm_trilinear_softargmin_stats_fwd"][1]) == len(P["ecm_trilinear_softargmin_fwd"][1]) + 1
    assert len(P["ecm_aggregate9_stats_fwd"][1]) == 12


def test_null_pointers_are_rejected_without_touching_the_gpu(lib_mod):
    lib = lib_mod.load()
    assert lib.ecm_softargmin_heads_lse_fwd(None, 1, None, None, 1, 1, 1, 1, None) == -1
    assert lib.ecm_aggregate9_stats_fwd(None, 1, None, None, None, 1, 1, 1, 1, 1, 4, None) == -1
    assert lib.ecm_volume_mapping_stats_fwd(None, 1, None, None, None, None, 1, 1, 1, 1, 1, 4, None) == -1
    assert lib.ecm_trilinear_softargmin_stats_fwd(None, 1, None, None, 1, 1, 1, 1, 1, 4, 4, 4, None) == -1


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 5, 12, 192])
def test_uniform_logits(D):
    _, std, peak, ent = logits_stats(torch.full((1, 1, D, 2, 3), 0.25, dtype=torch.float64))
    assert torch.allclose(std, torch.full_like(std, math.sqrt((D * D - 1) / 12)), rtol=1e-13, atol=1e-13)
    assert torch.allclose(peak, torch.full_like(peak, 1 / D), rtol=1e-13)
    assert torch.allclose(ent, torch.full_like(ent, math.log(D)), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("D,d1,d2", [(12, 2, 9), (48, 0, 47), (5, 3, 4)])
def test_two_equal_spikes(D, d1, d2):
    mu, std, peak, ent = logits_stats(spikes(D, (d1, d2)))
    assert abs(float(mu) - (d1 + d2) / 2) < 1e-12 * D
    assert abs(float(std) - abs(d1 - d2) / 2) < 1e-12 * D
    assert abs(float(peak) - 0.5) < 1e-12 and abs(float(ent) - math.log(2)) < 1e-12


def test_one_spike():
    mu, std, peak, ent = logits_stats(spikes(12, (7,)))
    assert abs(float(mu) - 7) < 1e-12 and 0 <= float(std) < 1e-10               # exp(-60) = 8.8e-27 on the eleven others
    assert 0 <= 1 - float(peak) < 1e-15 and 0 <= float(ent) < 1e-20


def _eight_case(NH=3, B=2, D=5, h=3, w=5, s=4, scale=1.5):
    c = seeded("hs.cpu.c", NH, B, D, h, w, scale=scale).double()
    w9 = torch.softmax(seeded("hs.cpu.w9", B, 9, h * s, w * s), 1).double()
    return c, w9, s


def test_eight_with_a_one_hot_centre_is_the_cell_itself():
    c, _, s = _eight_case()
    NH, B, D, h, w = c.shape
    disp, std, peak, ent = eight_t(c, one_hot_w9(B, h * s, w * s), s)
    mu, std_c, peak_c, ent_c = moments(F.softmax(cumulative(c), 2), 2)
    up = lambda t: t.repeat_interleave(s, -1).repeat_interleave(s, -2)                # noqa: E731
    assert torch.allclose(disp, s * up(mu), rtol=0, atol=1e-13)
    assert torch.allclose(std, s * up(std_c), rtol=0, atol=1e-13)
    assert torch.equal(peak, up(peak_c)) and torch.allclose(ent, up(ent_c), rtol=0, atol=1e-14)


def test_mixture_std_is_the_law_of_total_variance():
    c, w9, s = _eight_case()
    p, _, p_lr, a = eight_mixture(c, w9, s)
    NH, B, D, h, w = c.shape
    mu, std, _, _ = moments(p, 2)
    mu_c, std_c, _, _ = moments(p_lr, 2)
    mp, vp = F.pad(mu_c, (1, 1, 1, 1)), F.pad(std_c ** 2, (1, 1, 1, 1))
    var = 0
    for n, (dy, dx) in enumerate(NBR9):
        cut = lambda t: t[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w].repeat_interleave(s, -1).repeat_interleave(s, -2)   # noqa: E731
        var = var + a[:, n].unsqueeze(0) * (cut(vp) + (cut(mp) - mu) ** 2)
    assert torch.allclose(std, var.sqrt(), rtol=0, atol=1e-13)
    assert torch.allclose(p.sum(2), torch.ones_like(mu), rtol=0, atol=1e-14)


@pytest.mark.parametrize("h,w", [(3, 5), (1, 1), (1, 4), (2, 1)])
def test_mixture_mean_is_the_oracles_aggregate(h, w):
    """s * (sum of the valid weights) * mixture mean == ecm_aggregate9 of the soft-argmin disparities, border cells included
    (there the valid weights sum to less than one: the mixture renormalises, the head does not)."""
    c, w9, s = _eight_case(h=h, w=w)
    disp = eight_t(c, w9, s)[0]
    L = cumulative(c)
    want = torch.stack([O.ecm_aggregate_eight(O.soft_argmin(L[k]), w9, s)[:, 0] for k in range(c.shape[0])], 0)
    assert torch.allclose(disp, want, rtol=0, atol=1e-12 * float(want.abs().max()))
    border = ~valid9(h, w, s, "cpu").all(0)
    assert border.any() and float((w9 * valid9(h, w, s, "cpu")).sum(1)[:, border].max()) < 1


def test_volume_logits_are_the_established_closed_form():
    NH, B, Dl, h, w, s = 2, 2, 3, 2, 3, 4
    c = seeded("hs.cpu.vc", NH, B, Dl, h, w, scale=1.5).double()
    m5, mt3 = seeded("hs.cpu.m5", B, 5, h * s, w * s, scale=0.5).double(), seeded("hs.cpu.mt3", B, 3, h * s, w * s, scale=0.5).double()
    disp = volume_t(c, m5, mt3, s)[0]
    for k, L in enumerate(cumulative(c)):
        assert torch.equal(disp[k], volume_mapping_t(L, m5, mt3, s))
        assert torch.allclose(disp[k], O.volume_mapping(L, m5, mt3, s, Dl * s), rtol=0, atol=1e-12)
        assert torch.equal(soft_argmin_t(volume_logits_t(L, m5, mt3, s)), disp[k])


def test_trilinear_restatement_is_the_oracles_head():
    c = seeded("hs.cpu.tc", 2, 1, 3, 2, 3, scale=1.5).double()
    disp = trilinear_t3(c, 12, 7, 11)[0]
    for k, L in enumerate(cumulative(c)):
        assert torch.allclose(disp[k], O.trilinear_head(L, 12, 7, 11), rtol=0, atol=1e-12)


# ---- predict() refuses where no distribution exists, before any device work ----------------------------------------------------------
@pytest.mark.parametrize("name,why", [("cmfsm_sub_8", "do not sum to one"), ("cmf", "refinement decoder")])
def test_predict_refuses_heads_without_a_distribution(name, why):
    import ecm_amd
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(NotImplementedError, match=why):
        ecm_amd.get_model(name).predict(x, x)


def test_predict_checks_its_head_selection_on_the_cpu():
    import ecm_amd
    x = torch.zeros(1, 3, 64, 128)
    for bad in ((), (3,), (-1, 0)):
        with pytest.raises(ValueError, match="heads"):
            ecm_amd.get_model("cm_sub_8").predict(x, x, heads=bad)
