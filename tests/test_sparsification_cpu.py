"""Sparsification curves, the part that needs no GPU: `sparsify_t` below, a torch restatement of the
definition on the CPU -- the reference of tests/test_hip_sparsification.py -- checked against closed forms and against `brute`,
an independent statement in exact rational arithmetic; then the ABI additions, the size query and every refusal that comes before
any device work.

Definition, per sample: valid = 0 < gt < maxdisp, n of them; e = |pred - gt| in fp32 enters every sum as the integer
E = rint(min(e, 4095) * 65536) (NaN takes the clamp); bad = not (e < 3 or e < 0.05f * gt).  The key of a measure value is its
order-preserving 32-bit image (-0.0 as +0.0, NaN = 0xFFFFFFFF: removed first); the oracle's key is E.  For r_j = floor(j n / steps),
with A the groups of equal key strictly above the group (c, E_t, bad_t) holding rank r_j (from the highest key down) and
t = r_j - n_A, in fp64 and in this order:
    remE = (E_tot - E_A) - t * E_t / c;  rembad = (bad_tot - bad_A) - t * bad_t / c
    epe_j = (float)(remE / (n - r_j) / 65536);  d1_j = (float)(100 * rembad / (n - r_j))
and the oracle's d1 column is (float)(100 * (bad_tot - min(r_j, bad_tot)) / (n - r_j)).  n = 0: NaN.

sparsify_t does it with a stable full sort of the 64-bit keys and int64 cumulative sums."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

NEW_ENTRIES = ("ecm_eval_sparsify", "ecm_eval_sparsify_scratch_bytes", "ecm_eval_sparsify_max_measures", "ecm_eval_sparsify_max_steps")
NAN, INF = float("nan"), float("inf")
SIGN, MASK = 1 << 31, (1 << 32) - 1
CLAMP = 4095 * 65536
ULP = 2.0 ** -23


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def measure_key(u):
    """The int64 key of the fp32 values u."""
    bits = u.contiguous().view(torch.int32).long() & MASK
    bits = torch.where(u == 0, torch.zeros_like(bits), bits)
    key = torch.where(bits >= SIGN, MASK - bits, bits | SIGN)
    return torch.where(torch.isnan(u), torch.full_like(key, MASK), key)


def pixel_terms(pred, gt, maxdisp):
    """(mask, E int64, bad int64) of one sample's flat fp32 planes, the last two over the masked pixels."""
    mask = (gt > 0) & (gt < maxdisp)
    g = gt[mask]
    e = (pred[mask] - g).abs()
    ec = torch.where(e < 4095.0, e, torch.full_like(e, 4095.0))           # a NaN error takes the clamp
    E = torch.round(ec * 65536.0).to(torch.int64)                        # half to even, as rintf
    bad = ~((e < 3.0) | (e < torch.tensor(0.05, dtype=torch.float32) * g))
    return mask, E, bad.to(torch.int64)


def curve_t(key, E, bad, steps):
    """[steps,2] fp32 (epe_j, d1_j) of the n > 0 pixels with int64 keys `key`, on key's device."""
    n = key.numel()
    ks, order = torch.sort(key, descending=True, stable=True)
    cE, cbad = torch.cumsum(E[order], 0), torch.cumsum(bad[order], 0)
    Etot, badtot = cE[-1], cbad[-1]
    r = torch.tensor([j * n // steps for j in range(steps)], dtype=torch.int64, device=key.device)
    up = -ks                                                             # ascending
    lo, hi = torch.searchsorted(up, up[r].contiguous(), right=False), torch.searchsorted(up, up[r].contiguous(), right=True)
    zero = torch.zeros(1, dtype=torch.int64, device=key.device)
    cE0, cbad0 = torch.cat([zero, cE]), torch.cat([zero, cbad])           # exclusive sums: [i] = the sum of the first i
    EA, badA = cE0[lo], cbad0[lo]
    Et, badt = cE0[hi] - EA, cbad0[hi] - badA
    c, t = (hi - lo).double(), (r - lo).double()
    rest = (n - r).double()
    remE = (Etot - EA).double() - t * Et.double() / c
    rembad = (badtot - badA).double() - t * badt.double() / c
    return torch.stack([(remE / rest / 65536.0).float(), (100.0 * rembad / rest).float()], 1)


def sparsify_t(pred, gt, measures, maxdisp=192, steps=20):
    """(table fp32 [B,K+1,steps,2], count int64 [B,3]) of CPU tensors."""
    pred = pred[:, 0] if pred.dim() == 4 else pred
    measures = [m[:, 0] if m.dim() == 4 else m for m in measures]
    B, K = pred.shape[0], len(measures)
    table = torch.full((B, K + 1, steps, 2), NAN)
    count = torch.zeros(B, 3, dtype=torch.int64)
    for b in range(B):
        mask, E, bad = pixel_terms(pred[b].reshape(-1), gt[b].reshape(-1), maxdisp)
        n, badtot = E.numel(), int(bad.sum())
        count[b] = torch.tensor([n, int(E.sum()), badtot])
        if n == 0:
            continue
        for k, m in enumerate(measures):
            table[b, k] = curve_t(measure_key(m[b].reshape(-1)[mask]), E, bad, steps)
        table[b, K] = curve_t(E, E, bad, steps)
        for j in range(steps):
            r = j * n // steps
            table[b, K, j, 1] = torch.tensor(100.0 * float(badtot - min(r, badtot)) / float(n - r), dtype=torch.float64).float()
    return table, count


def areas_t(table):
    """(ause_epe, ause_d1, aurg_epe, aurg_d1), each [B,K] fp32, from a table."""
    t = table.double()
    curve, oracle = t[:, :-1], t[:, -1:]
    ause, aurg = (curve - oracle).mean(2), (curve[:, :, :1] - curve).mean(2)
    return ause[..., 0].float(), ause[..., 1].float(), aurg[..., 0].float(), aurg[..., 1].float()


def brute(pred, gt, measure, maxdisp, steps):
    """One sample, one measure, in exact rational arithmetic from Python floats: [(epe_j, d1_j)] as Fractions, or None if n = 0.
    The key order is stated again here without bit tricks: NaN above everything, then by value, -0.0 equal to +0.0."""
    import math
    import numpy as np
    f32 = np.float32
    rows = []
    for p, g, u in zip(pred, gt, measure):
        p, g, u = f32(p), f32(g), f32(u)
        if not (g > 0 and g < maxdisp):
            continue
        with np.errstate(all="ignore"):
            e = abs(f32(p - g))
            E = CLAMP if not e < f32(4095.0) else int(np.rint(f32(e * f32(65536.0))))
            bad = 0 if (e < f32(3.0) or e < f32(0.05) * g) else 1
        rank = (2, 0.0) if math.isnan(u) else (1, float(u) + 0.0)
        rows.append((rank, E, bad))
    n = len(rows)
    if n == 0:
        return None
    rows.sort(key=lambda row: row[0], reverse=True)
    out = []
    for j in range(steps):
        r = j * n // steps
        grp = [row for row in rows if row[0] == rows[r][0]]
        above = [row for row in rows if row[0] > rows[r][0]]
        t, c = r - len(above), len(grp)
        remE = sum(row[1] for row in rows) - sum(row[1] for row in above) - Fraction(t * sum(row[1] for row in grp), c)
        rembad = sum(row[2] for row in rows) - sum(row[2] for row in above) - Fraction(t * sum(row[2] for row in grp), c)
        out.append((remE / (n - r) / 65536, 100 * rembad / (n - r)))
    return out


def close_to_exact(got, want):
    """got [steps,2] fp32 against Fractions: within 1 fp32 ulp of the exact value (one fp64 chain, one rounding to fp32)."""
    for j, (epe, d1) in enumerate(want):
        for v, w in ((float(got[j, 0]), float(epe)), (float(got[j, 1]), float(d1))):
            assert abs(v - w) <= ULP * abs(w) + 1e-45, (j, v, w)


def kernel_constants():
    """The constexpr ints of csrc/eval_sparsify.hip by name."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "eval_sparsify.hip")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr):
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


def random_case(seed, shape, maxdisp=192.0):
    """(pred, gt) [B,H,W]: disparities in (0, maxdisp) with every 5th pixel invalid (0, negative or beyond), errors of up to a few
    pixels with every 7th much larger."""
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=gen) * (maxdisp - 2) + 1
    flat = gt.view(-1)
    flat[::15] = 0.0
    flat[5::15] = maxdisp + 3
    flat[10::15] = -4.0
    pred = gt + torch.randn(shape, generator=gen) * 1.5
    pred.view(-1)[::7] += 20.0
    return pred, gt


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_equal_measures_give_the_overall_mean_and_rate():
    pred, gt = random_case(1, (2, 9, 13))
    const = torch.full_like(gt, 0.25)
    table, count = sparsify_t(pred, gt, [const, torch.zeros_like(gt), torch.full_like(gt, NAN)], steps=7)
    for b in range(2):
        n, Etot, badtot = (int(v) for v in count[b])
        assert n == int(((gt[b] > 0) & (gt[b] < 192)).sum()) and 0 < badtot < n
        epe, d1 = Etot / n / 65536.0, 100.0 * badtot / n
        assert torch.allclose(table[b, :3, :, 0].double(), torch.tensor(epe, dtype=torch.float64), rtol=ULP, atol=0)
        assert torch.allclose(table[b, :3, :, 1].double(), torch.tensor(d1, dtype=torch.float64), rtol=ULP, atol=0)
    ause_epe, _, aurg_epe, aurg_d1 = areas_t(table)
    assert bool((ause_epe > 0).all()) and bool((aurg_epe.abs() < 1e-6).all()) and bool((aurg_d1.abs() < 1e-4).all())


def test_a_measure_that_rises_with_the_error_is_the_oracle():
    gen = torch.Generator().manual_seed(2)
    n = 300
    k = torch.randperm(5000, generator=gen)[:n].float() + 1                # distinct E = k: e = k / 65536 exactly
    gt = torch.full((1, 1, n), 50.0)
    pred = gt + (k / 65536.0 * 4096).view(1, 1, n)                        # e = k / 16 px, exact in fp32: E = 4096 k, distinct
    e = (pred - gt).abs()
    table, count = sparsify_t(pred, gt, [e, e * e + 1, -1.0 / (e + 1)], steps=20)
    assert int(count[0, 0]) == n and int(count[0, 1]) == int(k.sum()) * 4096
    for m in range(3):
        assert torch.equal(table[0, m, :, 0].view(torch.int32), table[0, 3, :, 0].view(torch.int32))
    # without ties the pro-rata d1 is the count of bad pixels left: the closed form, since the largest errors are the bad ones
    assert torch.equal(table[0, 0, :, 1].view(torch.int32), table[0, 3, :, 1].view(torch.int32))
    assert bool((areas_t(table)[0] == 0).all()) and bool((areas_t(table)[2] > 0).all())


@pytest.mark.parametrize("c,n,steps", [(1, 64, 8), (3, 1000, 20), (4096, 50, 64)])
def test_ramp(c, n, steps):
    k = torch.arange(1, n + 1, dtype=torch.float32)
    gt = torch.full((1, 1, n), 100.0)
    pred = gt - (k * c / 65536.0).view(1, 1, n)
    e = (pred - gt).abs()
    assert torch.equal((e * 65536).view(-1), k * c)                      # the errors are exact
    table, _ = sparsify_t(pred, gt, [e], steps=steps)
    for j in range(steps):
        left = n - j * n // steps                                        # k = 1..left stay: mean c (left + 1) / 2 / 65536
        want = c * (left + 1) / 2 / 65536.0
        assert abs(float(table[0, 0, j, 0]) - want) <= ULP * want and table[0, 0, j, 0] == table[0, 1, j, 0]


def test_one_step_one_pixel_and_none():
    pred, gt = random_case(3, (1, 4, 6))
    table, count = sparsify_t(pred, gt, [pred], steps=1)
    n, Etot, badtot = (int(v) for v in count[0])
    assert table.shape == (1, 2, 1, 2) and float(table[0, 0, 0, 0]) == float(torch.tensor(Etot / n / 65536.0).float())
    assert float(table[0, 1, 0, 1]) == float(torch.tensor(100.0 * badtot / n).float())
    gt1 = torch.zeros(1, 2, 3)
    gt1[0, 1, 1] = 7.0
    pred1 = torch.full((1, 2, 3), 9.5)
    table, count = sparsify_t(pred1, gt1, [pred1, -pred1], steps=5)
    assert count.tolist() == [[1, int(2.5 * 65536), 0]]                  # 2.5 px is under the 3-px bound
    assert bool((table[..., 0] == 2.5).all()) and bool((table[..., 1] == 0).all())      # floor(j / 5) = 0: nothing is removed
    table, count = sparsify_t(pred1, torch.zeros(1, 2, 3), [pred1], steps=4)
    assert count.tolist() == [[0, 0, 0]] and bool(torch.isnan(table).all())
    table, _ = sparsify_t(torch.cat([pred1, pred1]), torch.cat([torch.zeros(1, 2, 3), gt1]), [torch.cat([pred1, pred1])], steps=3)
    assert bool(torch.isnan(table[0]).all()) and bool((table[1, :, :, 0] == 2.5).all())


def tie_case():
    """20 valid pixels, steps = 4: r = 0, 5, 10, 15.  Measure groups from the top: 5 pixels (r_1 = 5 is the first of the next group:
    t = 0), then 6 (r_2 = 10 is its last: t = c - 1), then 9 (r_3 = 15: inside)."""
    measure = torch.tensor([9.0] * 5 + [4.0] * 6 + [-1.0] * 9)
    perm = torch.randperm(20, generator=torch.Generator().manual_seed(4))
    gt = torch.full((20,), 30.0)
    pred = gt + torch.linspace(0.0, 9.5, 20)
    return pred[perm].view(1, 1, 20), gt.view(1, 1, 20), measure[perm].view(1, 1, 20)


def test_cuts_on_and_beside_a_group_boundary():
    pred, gt, measure = tie_case()
    table, _ = sparsify_t(pred, gt, [measure], steps=4)
    close_to_exact(table[0, 0], brute(pred.view(-1).tolist(), gt.view(-1).tolist(), measure.view(-1).tolist(), 192, 4))
    _, E, bad = pixel_terms(pred.view(-1), gt.view(-1), 192)
    m = measure.view(-1)
    # t = 0: exactly the top group is gone
    left = m < 9.0
    assert float(table[0, 0, 1, 0]) == float((E[left].sum().double() / 15 / 65536.0).float())
    assert float(table[0, 0, 1, 1]) == float((100.0 * bad[left].sum().double() / 15).float())
    # t = c - 1 = 5: the top group and five sixths of the second
    want = (E.sum() - E[m == 9.0].sum()).double() - 5.0 * E[m == 4.0].sum().double() / 6.0
    assert float(table[0, 0, 2, 0]) == float((want / 10 / 65536.0).float())


def test_zeros_infinities_and_nan_as_measures():
    # keys, from the top: NaN, +inf, 1, +-0 (one group), -1, -inf
    measure = torch.tensor([0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, -0.0, 0.0, NAN])
    assert measure_key(torch.tensor([-0.0])).item() == measure_key(torch.tensor([0.0])).item() == SIGN
    assert measure_key(torch.tensor([NAN])).item() == measure_key(-torch.tensor([NAN])).item() == MASK
    keys = measure_key(torch.tensor([-INF, -1.0, 0.0, 1e-45, 1.0, INF, NAN])).tolist()
    assert keys == sorted(keys) and len(set(keys)) == 7
    gt = torch.full((10,), 20.0)
    pred = gt + torch.arange(10, dtype=torch.float32)
    table, _ = sparsify_t(pred.view(1, 1, 10), gt.view(1, 1, 10), [measure.view(1, 1, 10)], steps=10)
    close_to_exact(table[0, 0], brute(pred.tolist(), gt.tolist(), measure.tolist(), 192, 10))
    # the two NaN go first (errors 4 and 9), then +inf (2), then 1.0 (5): mean of the rest after four removals
    assert float(table[0, 0, 4, 0]) == float(torch.tensor((45 - 4 - 9 - 2 - 5) / 6.0).float())
    # the four zeros are one group: after the fifth removal a quarter of their errors (0 + 1 + 7 + 8) is gone
    assert float(table[0, 0, 5, 0]) == float(torch.tensor((25 - 16 / 4.0) / 5.0).float())


def test_nan_and_oversized_predictions_take_the_clamp():
    gt = torch.full((1, 1, 6), 10.0)
    pred = torch.tensor([10.5, NAN, 1e9, INF, -INF, 4105.0 + 10]).view(1, 1, 6)
    table, count = sparsify_t(pred, gt, [torch.arange(6.0).view(1, 1, 6)], steps=6)
    assert count.tolist() == [[6, 32768 + 5 * CLAMP, 5]]
    assert float(table[0, 0, 0, 0]) == float(torch.tensor((0.5 + 5 * 4095.0) / 6).float()) and float(table[0, 0, 5, 0]) == 0.5
    assert float(table[0, 1, 5, 0]) == 0.5 and float(table[0, 1, 1, 0]) == float(torch.tensor((0.5 + 4 * 4095.0) / 5).float())
    assert not bool(torch.isnan(table).any())


def test_oracle_d1_against_brute_force():
    pred, gt = random_case(5, (1, 11, 17))
    table, count = sparsify_t(pred, gt, [pred], steps=13)
    mask, E, bad = pixel_terms(pred.view(-1), gt.view(-1), 192)
    flags = sorted(bad.tolist(), reverse=True)                           # the bad pixels leave first
    n = len(flags)
    for j in range(13):
        r = j * n // 13
        want = torch.tensor(100.0 * sum(flags[r:]) / (n - r), dtype=torch.float64).float()
        assert float(table[0, 1, j, 1]) == float(want)
    assert int(count[0, 2]) == sum(flags)
    # and a random measure against the exact statement
    gen = torch.Generator().manual_seed(6)
    measure = torch.randint(0, 9, gt.shape, generator=gen).float() - 4
    table, _ = sparsify_t(pred, gt, [measure], steps=13)
    close_to_exact(table[0, 0], brute(pred.view(-1).tolist(), gt.view(-1).tolist(), measure.view(-1).tolist(), 192, 13))


def test_maxdisp_bounds_the_mask():
    pred, gt = random_case(7, (1, 6, 9))
    t192, c192 = sparsify_t(pred, gt, [pred], maxdisp=192, steps=3)
    t64, c64 = sparsify_t(pred, gt, [pred], maxdisp=64, steps=3)
    assert int(c64[0, 0]) == int(((gt > 0) & (gt < 64)).sum()) < int(c192[0, 0])


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
    assert lib_mod.query("ecm_abi_version") >= 15
    assert len(lib_mod.PROTOTYPES["ecm_eval_sparsify"][1]) == 14 and len(lib_mod.PROTOTYPES["ecm_eval_sparsify_scratch_bytes"][1]) == 5


def test_limits_and_the_size_query_need_no_gpu(lib_mod):
    import ecm_amd
    k = kernel_constants()
    assert ecm_amd.ops.eval_sparsification_limits() == (8, 64) == (k["MAX_K"], k["MAX_STEPS"])
    assert k["DIGIT"] * k["LEVELS"] == 32 and k["BINS"] == 1 << k["DIGIT"] and k["SPAN"] == k["ST"] * k["PER_THREAD"]
    q = lambda *a: lib_mod.query("ecm_eval_sparsify_scratch_bytes", *a)          # noqa: E731
    base = q(2, 32, 64, 3, 20)
    assert base > 0 and base % 8 == 0
    assert q(3, 32, 64, 3, 20) > base and q(2, 32, 64, 4, 20) > base and q(2, 32, 64, 3, 21) > base
    assert q(2, 33, 64, 3, 20) >= base and q(2, 32, 65, 3, 20) >= base
    for K in range(1, 9):                                                # rises with every argument that sizes it
        for steps in range(1, 65):
            here = q(2, 5, 7, K, steps)
            assert here > 0 and (steps == 1 or here > q(2, 5, 7, K, steps - 1)) and (K == 1 or here > q(2, 5, 7, K - 1, steps))
            assert here > q(1, 5, 7, K, steps)
    for bad in ((0, 4, 4, 1, 4), (1, 0, 4, 1, 4), (1, 4, 0, 1, 4), (1, 4, 4, 0, 4), (1, 4, 4, 9, 4), (1, 4, 4, 1, 0), (1, 4, 4, 1, 65)):
        assert q(*bad) == 0, bad


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    lib = lib_mod.load()
    p, big = C.c_void_p(4096), C.c_longlong(1 << 40)                      # never dereferenced: every call below returns first
    planes = (C.c_void_p * 9)(*([4096] * 9))
    call = lambda *a: lib.ecm_eval_sparsify(*a, C.c_float(192.0), None)          # noqa: E731
    assert call(None, p, planes, p, p, p, big, 1, 4, 4, 1, 4) == -1
    assert call(p, p, None, p, p, p, big, 1, 4, 4, 1, 4) == -1
    assert call(p, p, planes, None, p, p, big, 1, 4, 4, 1, 4) == -1
    assert call(p, p, planes, p, None, p, big, 1, 4, 4, 1, 4) == -1
    assert call(p, p, planes, p, p, None, big, 1, 4, 4, 1, 4) == -1
    assert call(p, p, planes, p, p, C.c_void_p(4100), big, 1, 4, 4, 1, 4) == -1        # scratch not 8-byte aligned
    for B, H, W, K, steps in ((0, 4, 4, 1, 4), (1, 0, 4, 1, 4), (1, 4, 0, 1, 4), (1, 4, 4, 0, 4), (1, 4, 4, 1, 0), (-1, 4, 4, 1, 4)):
        assert call(p, p, planes, p, p, p, big, B, H, W, K, steps) == -1
    for B, H, W, K, steps in ((1, 1 << 16, 1 << 15, 1, 4), (65536, 4, 4, 1, 4), (1, 4, 4, 9, 4), (1, 4, 4, 1, 65)):
        assert call(p, p, planes, p, p, p, big, B, H, W, K, steps) == -2
    holes = (C.c_void_p * 2)(4096, None)
    assert call(p, p, holes, p, p, p, big, 1, 4, 4, 2, 4) == -1
    need = lib_mod.query("ecm_eval_sparsify_scratch_bytes", 1, 4, 4, 1, 4)
    assert call(p, p, planes, p, p, p, C.c_longlong(need - 1), 1, 4, 4, 1, 4) == -3
    assert call(p, p, planes, p, p, p, C.c_longlong(0), 1, 4, 4, 1, 4) == -3


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
def test_op_refusals():
    import ecm_amd
    ops = ecm_amd.ops
    x = torch.zeros(1, 4, 8)
    sig = inspect.signature(ops.eval_sparsification)
    assert list(sig.parameters) == ["pred", "gt", "measures", "maxdisp", "steps"]
    assert sig.parameters["maxdisp"].default == 192 and sig.parameters["steps"].default == 20
    assert ops.Sparsification._fields == ("epe", "d1", "oracle_epe", "oracle_d1", "ause_epe", "ause_d1", "aurg_epe", "aurg_d1", "count")
    with pytest.raises(ValueError, match="measures"):
        ops.eval_sparsification(x, x, [])
    with pytest.raises(ValueError, match="measures"):
        ops.eval_sparsification(x, x, [x] * 9)
    for bad in (0, 65, -1, 2.0, True, None, "20"):
        with pytest.raises(ValueError, match="steps"):
            ops.eval_sparsification(x, x, [x], steps=bad)
    for bad in (0, -1.0, NAN, INF, None, True):
        with pytest.raises(ValueError, match="maxdisp"):
            ops.eval_sparsification(x, x, [x], maxdisp=bad)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.eval_sparsification(x, x, [x])

    class OnDevice(torch.Tensor):
        """A CPU tensor that says it is on the device: the shape and dtype contract is checked before anything is launched."""
        is_cuda = True

    fake = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)     # noqa: E731
    ok = fake(1, 4, 8)
    for pred, gt, ms in ((fake(4, 8), fake(4, 8), [fake(4, 8)]), (fake(1, 2, 4, 8), ok, [ok]), (ok, fake(1, 4, 9), [ok]),
                         (fake(1, 0, 8), fake(1, 0, 8), [fake(1, 0, 8)]), (ok, ok, [fake(1, 4, 9)]), (ok, ok, [ok, fake(2, 4, 8)]),
                         (ok, fake(1, 1, 4, 8), [ok])):
        with pytest.raises(RuntimeError, match="eval_sparsification"):
            ops.eval_sparsification(pred, gt, ms)
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match="fp32"):
            ops.eval_sparsification(ok, ok, [fake(1, 4, 8, dtype=dtype)])
        with pytest.raises(RuntimeError, match="fp32"):
            ops.eval_sparsification(fake(1, 4, 8, dtype=dtype), ok, [ok])
    with pytest.raises(ValueError, match="65535"):
        ops.eval_sparsification(fake(65536, 1, 1), fake(65536, 1, 1), [fake(65536, 1, 1)])
    # the areas are plain torch
    table, _ = sparsify_t(*random_case(8, (2, 5, 6)), [random_case(9, (2, 5, 6))[0]], steps=4)
    ause, aurg = ops.sparsification_areas(table[:, :1, :, 0], table[:, 1, :, 0])
    assert ause.dtype == torch.float64 and torch.equal(ause.float(), areas_t(table)[0]) and torch.equal(aurg.float(), areas_t(table)[2])


def test_model_refusals():
    import ecm_amd
    from ecm_amd import models
    assert models.SPARSIFICATION_MEASURES == ("std", "entropy", "peak", "mass")
    sig = inspect.signature(models._ECMNet.sparsification)
    assert list(sig.parameters) == ["self", "left", "right", "gt", "head", "measures", "mode_radius", "steps", "maxdisp"]
    assert [sig.parameters[n].default for n in ("head", "measures", "mode_radius", "steps", "maxdisp")] == [2, ("std", "entropy", "peak"), None, 20, 192]
    x, gt = torch.zeros(1, 3, 64, 128), torch.zeros(1, 64, 128)            # CPU tensors: a forward on them raises RuntimeError
    net = ecm_amd.get_model("cmfsm")
    for bad in (("std", "variance"), ("mass",), ("std", "mass"), (), "disparity", ("std",) * 9):
        with pytest.raises(ValueError, match="measure"):
            net.sparsification(x, x, gt, measures=bad)
    with pytest.raises(ValueError, match="measure"):
        net.sparsification(x, x, gt, measures=("mode",), mode_radius=8)
    for bad in (-1, 3, True, 1.0):
        with pytest.raises(ValueError, match="head"):
            net.sparsification(x, x, gt, head=bad)
    with pytest.raises(ValueError, match="steps"):
        net.sparsification(x, x, gt, steps=0)
    with pytest.raises(ValueError, match="steps"):
        net.sparsification(x, x, gt, steps=65)
    with pytest.raises(ValueError, match="maxdisp"):
        net.sparsification(x, x, gt, maxdisp=0)
    with pytest.raises(ValueError, match="radius"):
        net.sparsification(x, x, gt, measures=("mass",), mode_radius=-1)
    with pytest.raises(RuntimeError):                                    # everything is in order: the forward refuses CPU tensors
        net.sparsification(x, x, gt, measures=("std", "mass"), mode_radius=8)
    for arch in ("cmf", "cmfsm_sub_8"):
        with pytest.raises(NotImplementedError, match="predict"):
            ecm_amd.get_model(arch).sparsification(x, x, gt)
    assert all(hasattr(cls, "sparsification") for cls in models._MODELS.values())


def test_dataset_curves_are_the_mean_over_samples_with_valid_pixels():
    from importlib import import_module
    dist = import_module("explicit-context-mapping-for-stereo-matching_amd.dist")
    pred, gt = random_case(10, (3, 5, 8))
    gt[1] = 0.0                                                          # a sample without valid pixels
    table, count = sparsify_t(pred, gt, [pred, -pred], steps=5)
    res = dist.sparsification_dataset(table, count)
    assert res["samples"] == 2 and res["epe"].dtype == torch.float64 and res["epe"].shape == (2, 5) and res["oracle_d1"].shape == (5,)
    want = table.double()[[0, 2]].mean(0)
    assert torch.equal(res["epe"], want[:2, :, 0]) and torch.equal(res["oracle_d1"], want[2, :, 1])
    assert torch.equal(res["ause_d1"], (want[:2, :, 1] - want[2:, :, 1]).mean(1)) and torch.equal(res["aurg_epe"], (want[:2, :1, 0] - want[:2, :, 0]).mean(1))
    empty = dist.sparsification_dataset(table[1:2], count[1:2])
    assert empty["samples"] == 0 and bool(torch.isnan(empty["epe"]).all())
    sig = inspect.signature(dist.evaluate_sparsification)
    assert list(sig.parameters) == ["model", "batches", "head", "measures", "mode_radius", "steps", "maxdisp"]
