"""Sparsification curves on the MI355X: ops.eval_sparsification, _ECMNet.sparsification and
dist.evaluate_sparsification against sparsify_t, the CPU restatement of tests/test_sparsification_cpu.py.

`count` compares bit for bit: it is integer.  `table` compares within 1 fp32 ulp (measured as the distance of the bit patterns),
which is derived, not measured: both sides evaluate the same fp64 expression, in the same order, from the same integers, and
round once to fp32; the one ulp is for a compiler that forms an fp64 quotient differently.  Every test prints the distance it saw.

Shapes are the smallest at which the kernel can go wrong: 1x5x7 (one wave, partly filled), 2x33x67 (odd width: 4-byte loads,
two workgroups per sample), 2x32x64 (16-byte loads) and the same data one element off alignment (4-byte loads again); SPAN - 1,
SPAN, SPAN + 1 pixels; more spans than the per-sample workgroup cap, so that a workgroup walks on to a second span.  The radix
levels are driven by measures built from bit patterns: keys that differ only in one of the four digits."""
from importlib import import_module

import pytest
import torch

from test_hip_guard_bands import POISON, guarded
from test_sparsification_cpu import INF, NAN, areas_t, kernel_constants, random_case, sparsify_t, tie_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KC = kernel_constants()


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def bits(t):
    return t.contiguous().view(torch.int32)


def table_of(sp):
    """[B,K+1,steps,2] from a Sparsification."""
    return torch.cat([torch.stack([sp.epe, sp.d1], -1), torch.stack([sp.oracle_epe, sp.oracle_d1], -1).unsqueeze(1)], 1)


def ulp_distance(got, want):
    """The largest distance of the fp32 bit patterns (all values are >= 0 or NaN; NaN must meet NaN)."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "NaN rows differ"
    if bool(gn.all()):
        return 0
    return int((bits(got).long() - bits(want).long())[~gn].abs().max())


def off_by_one(t):
    """The same values at an address that is 4 bytes past a 16-byte boundary."""
    raw = torch.empty(t.numel() + 4, device=DEV, dtype=t.dtype)
    at = 1 + (-(raw.data_ptr() // 4)) % 4
    out = raw[at:at + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def assert_parity(ecm, pred, gt, measures, steps=20, maxdisp=192, what="", place=None):
    want_table, want_count = sparsify_t(pred, gt, measures, maxdisp, steps)
    place = place or (lambda t: t.to(DEV))
    sp = ecm.ops.eval_sparsification(place(pred), place(gt), [place(m) for m in measures], maxdisp, steps)
    B, K = pred.shape[0], len(measures)
    assert sp.epe.shape == sp.d1.shape == (B, K, steps) and sp.oracle_epe.shape == sp.oracle_d1.shape == (B, steps)
    assert sp.count.dtype == torch.int64 and sp.count.shape == (B, 3) and all(f.dtype == torch.float32 for f in sp[:8])
    count, table = sp.count.cpu(), table_of(sp).cpu()
    assert torch.equal(count, want_count), f"{what}: count {count.tolist()} != {want_count.tolist()}"
    d = ulp_distance(table, want_table)
    print(f"SPARSIFY {what}: {d} ulp")
    assert d <= 1, f"{what}: table differs by {d} ulp"
    for got, want in zip(sp[4:8], areas_t(table)):                       # fp64 means of <= 64 terms of at most 4095, rounded once
        assert got.shape == (B, K) and torch.allclose(got.cpu(), want, rtol=2.0 ** -22, atol=1e-9, equal_nan=True), what
    return sp


def measures_for(pred, gt, seed):
    """Three planes: general floats of both signs, a quantised one (large tie groups), and one that follows the error loosely."""
    gen = torch.Generator().manual_seed(seed)
    noise = torch.randn(pred.shape, generator=gen)
    return [noise * 3, torch.randint(0, 5, pred.shape, generator=gen).float() - 2, (pred - gt).abs() + noise.abs()]


def from_bits(pattern):
    return pattern.to(torch.int32).view(torch.float32)


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 33, 67), (2, 32, 64)], ids=lambda s: "x".join(map(str, s)))
def test_parity(ecm, shape):
    pred, gt = random_case(20 + shape[2], shape)
    ms = measures_for(pred, gt, 30 + shape[2])
    assert_parity(ecm, pred, gt, ms, what=f"{shape}")
    assert_parity(ecm, pred, gt, ms, steps=7, maxdisp=64, what=f"{shape} steps 7 maxdisp 64")
    assert_parity(ecm, pred, gt, ms, what=f"{shape} off alignment", place=lambda t: off_by_one(t.to(DEV)))
    assert_parity(ecm, pred.unsqueeze(1), gt, [m.unsqueeze(1) for m in ms], what=f"{shape} as [B,1,H,W]")
    ecm.ops.check_async_errors()


def test_the_two_load_widths_decide_alike(ecm):
    pred, gt = random_case(40, (2, 32, 64))
    ms = measures_for(pred, gt, 41)
    a = ecm.ops.eval_sparsification(pred.to(DEV), gt.to(DEV), [m.to(DEV) for m in ms])
    b = ecm.ops.eval_sparsification(off_by_one(pred.to(DEV)), off_by_one(gt.to(DEV)), [off_by_one(m.to(DEV)) for m in ms])
    c = ecm.ops.eval_sparsification(pred.to(DEV), gt.to(DEV), [ms[0].to(DEV), off_by_one(ms[1].to(DEV)), ms[2].to(DEV)])
    for other in (b, c):
        assert torch.equal(bits(table_of(a)), bits(table_of(other))) and torch.equal(a.count, other.count)


# ---- every radix level must decide -------------------------------------------------------------------------------------------------
def test_every_digit_decides(ecm):
    shape = (2, 24, 40)
    pred, gt = random_case(50, shape)
    gen = torch.Generator().manual_seed(51)
    digit = lambda: torch.randint(0, 256, shape, generator=gen)          # noqa: E731
    base = 0x41200000                                                    # 10.0: the low 20 bits are free
    ms = [from_bits(base | digit()),                                     # keys differ in the lowest digit only
          from_bits(base | (digit() << 8)),                              # in the third
          from_bits(base & 0xFF00FFFF | (digit() << 16)),                # in the second
          from_bits(base | digit() | (digit() << 8)),                    # in the two low ones
          from_bits(-(0x3F000000 | digit() | (digit() % 3 << 8))),       # sign bit set: the order of the bits is reversed
          from_bits(torch.randint(-(1 << 31), 1 << 31, shape, generator=gen))]    # any bit pattern: NaN, inf and denormals among them
    assert all(torch.isfinite(m).all() for m in ms[:4]) and bool(torch.isnan(ms[5]).any())
    assert_parity(ecm, pred, gt, ms, steps=20, what="digits")
    assert_parity(ecm, pred, gt, ms, steps=64, what="digits, 64 cuts")    # several cuts share a bin at every level
    ecm.ops.check_async_errors()


def test_cuts_that_share_a_bin_and_a_key(ecm):
    shape = (1, 16, 48)
    pred, gt = random_case(52, shape)
    gen = torch.Generator().manual_seed(53)
    three = torch.randint(0, 3, shape, generator=gen).float()            # three keys for 64 cuts: up to ~21 cuts per key
    near = from_bits(0x42000000 | torch.randint(0, 4, shape, generator=gen))      # four neighbouring keys of one bin at every level
    spread = torch.randn(shape, generator=gen) * 1e3
    spread.view(-1)[::11] = INF
    spread.view(-1)[3::11] = -INF
    spread.view(-1)[5::11] = NAN
    spread.view(-1)[7::11] = -0.0
    spread.view(-1)[8::11] = 0.0
    assert_parity(ecm, pred, gt, [three, near, spread], steps=64, what="shared bins")
    assert_parity(ecm, pred, gt, [three, near, spread], steps=5, what="shared bins, 5 cuts")
    ecm.ops.check_async_errors()


# ---- ties --------------------------------------------------------------------------------------------------------------------------
def test_ties(ecm):
    pred, gt, measure = tie_case()                                       # t = 0 at r_1 and t = c - 1 at r_2
    assert_parity(ecm, pred, gt, [measure, -measure], steps=4, what="tie group straddling a cut")
    pred, gt = random_case(54, (2, 9, 21))
    one = [torch.full_like(gt, 0.75), torch.zeros_like(gt), torch.full_like(gt, NAN), torch.full_like(gt, -INF)]
    sp = assert_parity(ecm, pred, gt, one, steps=9, what="the image as one group")
    assert torch.equal(bits(sp.epe[:, 0]), bits(sp.epe[:, 1])) and torch.equal(bits(sp.epe[:, 0]), bits(sp.epe[:, 3]))
    ecm.ops.check_async_errors()


# ---- the reduction grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_about_one_span(ecm, delta):
    hw = KC["SPAN"] + delta
    pred, gt = random_case(60 + delta, (2, 1, hw))
    assert_parity(ecm, pred, gt, measures_for(pred, gt, 61)[:2], steps=6, what=f"{hw} pixels")
    ecm.ops.check_async_errors()


def test_past_the_workgroup_cap(ecm):
    spans = KC["MAX_BLOCKS"] + 2
    for shape in ((1, spans, KC["SPAN"] - 4), (1, spans * KC["SPAN"] // 8 + 1, 8)):      # scalar loads with a ragged end; vector loads
        assert shape[1] * shape[2] > KC["MAX_BLOCKS"] * KC["SPAN"] and (shape[2] % 4 == 0)
        pred, gt = random_case(62, shape)
        place = (lambda t: off_by_one(t.to(DEV))) if shape[2] != 8 else None
        assert_parity(ecm, pred, gt, [measures_for(pred, gt, 63)[0]], steps=20, what=f"{shape}", place=place)
    ecm.ops.check_async_errors()


# ---- smaller checks ----------------------------------------------------------------------------------------------------------------
def test_masks(ecm):
    pred, gt = random_case(64, (2, 12, 20))
    ms = measures_for(pred, gt, 65)
    empty = torch.zeros_like(gt)
    sp = assert_parity(ecm, pred, empty, ms, what="empty mask")
    assert bool(torch.isnan(table_of(sp)).all()) and sp.count.tolist() == [[0, 0, 0]] * 2
    full = gt.clamp(1.0, 191.0)
    sp = assert_parity(ecm, pred, full, ms, what="full mask")
    assert sp.count[:, 0].tolist() == [240, 240]
    single = torch.zeros_like(gt)
    single[0, 3, 4], single[1, 11, 19] = 17.0, 5.0
    sp = assert_parity(ecm, pred, single, ms, what="one valid pixel")
    assert sp.count[:, 0].tolist() == [1, 1]
    beside = gt.clone()
    beside[0] = -1.0
    sp = assert_parity(ecm, pred, beside, ms, what="an empty sample beside a dense one")
    assert bool(torch.isnan(table_of(sp)[0]).all()) and not bool(torch.isnan(table_of(sp)[1]).any())
    ecm.ops.check_async_errors()


@pytest.mark.parametrize("K,steps", [(1, 1), (1, 64), (8, 1), (8, 64), (5, 33)])
def test_every_accepted_size(ecm, K, steps):
    pred, gt = random_case(66, (2, 10, 26))
    gen = torch.Generator().manual_seed(67)
    ms = [torch.randn(pred.shape, generator=gen).round() for _ in range(K)]
    assert_parity(ecm, pred, gt, ms, steps=steps, what=f"K {K} steps {steps}")
    ecm.ops.check_async_errors()


def test_the_error_as_a_measure_is_the_oracle(ecm):
    gen = torch.Generator().manual_seed(68)
    shape = (2, 16, 36)
    gt = torch.full(shape, 50.0)
    gt.view(-1)[::9] = 0.0
    k = torch.randint(0, 1 << 19, shape, generator=gen).float()          # e = k / 65536 < 8 px, exact beside gt = 50: E = k
    k.view(-1)[::5] = 12345.0                                            # ... with a tie group
    pred = gt + k / 65536.0
    e = (pred - gt).abs()
    assert torch.equal(e * 65536.0, k)
    sp = assert_parity(ecm, pred, gt, [e, -e], steps=20, what="the error as a measure")
    assert torch.equal(bits(sp.epe[:, 0]), bits(sp.oracle_epe)) and torch.equal(bits(sp.d1[:, 0]), bits(sp.oracle_d1))
    assert bool((sp.ause_epe[:, 0] == 0).all()) and bool((sp.ause_epe[:, 1] > 0).all()) and bool((sp.aurg_epe[:, 0] > 0).all())
    ecm.ops.check_async_errors()


def test_rows_do_not_depend_on_the_batch_and_runs_repeat(ecm):
    ops = ecm.ops
    pred, gt = random_case(69, (3, 33, 67))
    gt[1] = 0.0
    ms = measures_for(pred, gt, 70)
    pd, gd, md = pred.to(DEV), gt.to(DEV), [m.to(DEV) for m in ms]
    whole = ops.eval_sparsification(pd, gd, md, steps=11)
    again = ops.eval_sparsification(pd, gd, md, steps=11)
    assert torch.equal(bits(table_of(whole)), bits(table_of(again))) and torch.equal(whole.count, again.count)
    for f, g in zip(whole[4:8], again[4:8]):
        assert torch.equal(bits(f), bits(g))
    for b in range(3):
        alone = ops.eval_sparsification(pd[b:b + 1], gd[b:b + 1], [m[b:b + 1] for m in md], steps=11)
        assert torch.equal(bits(table_of(alone)[0]), bits(table_of(whole)[b])) and torch.equal(alone.count[0], whole.count[b])
    before = [t.clone() for t in (pd, gd, *md)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.eval_sparsification(pd, gd, md, steps=11)
    side.synchronize()
    assert torch.equal(bits(table_of(other)), bits(table_of(whole)))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, (pd, gd, *md)))      # the inputs are not written
    ops.check_async_errors()


def test_guard_bands_and_an_undersized_scratch(ecm):
    import ctypes as C
    ops, lib = ecm.ops, ecm._lib
    for shape, K, steps in (((1, 5, 7), 1, 1), ((2, 33, 67), 3, 20), ((2, 32, 64), 8, 64), ((1, 1, KC["SPAN"] + 1), 2, 5)):
        pred, gt = random_case(71, shape)
        ms = [m.to(DEV) for m in (measures_for(pred, gt, 72) * 3)[:K]]
        with guarded(ecm) as g:
            ops.eval_sparsification(pred.to(DEV), gt.to(DEV), ms, steps=steps)
            g.check(f"eval_sparsification {shape} K {K} steps {steps}")
            assert len(g.records) == 3                                   # table, count, scratch
    pred, gt = random_case(73, (2, 8, 12))
    pd, gd, md = pred.to(DEV), gt.to(DEV), pred.to(DEV)
    table = torch.full((2, 2, 4, 2), -7.0, device=DEV)
    count = torch.full((2, 3), -7, device=DEV, dtype=torch.int64)
    need = lib.query("ecm_eval_sparsify_scratch_bytes", 2, 8, 12, 1, 4)
    scratch = torch.full((need,), POISON, device=DEV, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())                               # noqa: E731
    ptrs = (C.c_void_p * 1)(md.data_ptr())
    with pytest.raises(RuntimeError, match="scratch"):
        lib.call("ecm_eval_sparsify", p(pd), p(gd), ptrs, p(table), p(count), p(scratch), C.c_longlong(need - 8), 2, 8, 12, 1, 4,
                 C.c_float(192.0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((table == -7.0).all()) and bool((count == -7).all()) and bool((scratch == POISON).all())
    lib.call("ecm_eval_sparsify", p(pd), p(gd), ptrs, p(table), p(count), p(scratch), C.c_longlong(need), 2, 8, 12, 1, 4,
             C.c_float(192.0), C.c_void_p(torch.cuda.current_stream().cuda_stream))       # the poisoned scratch is cleared by the call
    want_table, want_count = sparsify_t(pred, gt, [pred], steps=4)
    assert torch.equal(count.cpu(), want_count) and ulp_distance(table.cpu(), want_table) <= 1
    ops.check_async_errors()


# ---- the entry points --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(ecm):
    torch.manual_seed(5)
    model = ecm.get_model("cmfsm").to(DEV).eval()
    gen = torch.Generator(device=DEV).manual_seed(11)
    left, right = (torch.randn(2, 3, 256, 256, device=DEV, generator=gen) for _ in range(2))
    gt = torch.rand(2, 256, 256, device=DEV, generator=gen) * 200.0 - 4.0          # some pixels outside (0, 192)
    return model, left, right, gt


@pytest.mark.parametrize("radius,measures", [(None, ("std", "entropy", "peak")), (8, ("mass", "std", "peak"))])
def test_model_sparsification(ecm, net, radius, measures):
    model, left, right, gt = net
    left, right, gt = left[:1], right[:1], gt[:1]
    prediction, sp = model.sparsification(left, right, gt, measures=measures, mode_radius=radius, steps=10)
    plain = model.predict(left, right, (2,), radius)
    assert type(prediction) is type(plain) and type(sp).__name__ == "Sparsification"
    for a, b in zip(prediction, plain):
        assert len(a) == len(b) == 1 and torch.equal(bits(a[0]), bits(b[0]))
    planes = [getattr(plain, name)[0].cpu() * (-1.0 if name in ("peak", "mass") else 1.0) for name in measures]
    want_table, want_count = sparsify_t(plain.disparity[0].cpu(), gt.cpu(), planes, 192, 10)
    assert torch.equal(sp.count.cpu(), want_count) and 0 < int(want_count[0, 0]) < 256 * 256
    d = ulp_distance(table_of(sp).cpu(), want_table)
    print(f"SPARSIFY model {measures}: {d} ulp")
    assert d <= 1
    head0, _ = model.sparsification(left, right, gt, head=0, measures=("std",), steps=3)
    assert torch.equal(bits(head0.disparity[0]), bits(model.predict(left, right, (0,)).disparity[0]))
    ecm.ops.check_async_errors()


def test_architectures_without_a_distribution_raise(ecm):
    x, gt = torch.zeros(1, 3, 256, 512, device=DEV), torch.ones(1, 256, 512, device=DEV)
    for arch in ("cmf", "cmfsm_sub_8"):
        with pytest.raises(NotImplementedError, match="predict"):
            ecm.get_model(arch).to(DEV).sparsification(x, x, gt)
    with pytest.raises(ValueError, match="measure"):
        ecm.get_model("cmfsm").sparsification(x, x, gt, measures=("mass",))


def test_evaluate_sparsification(ecm, net, tmp_path):
    import torch.distributed as dist
    D = import_module("explicit-context-mapping-for-stereo-matching_amd.dist")
    model, left, right, gt = net
    batches = [(left[i:i + 1], right[i:i + 1], gt[i:i + 1], None) for i in range(2)]
    res = D.evaluate_sparsification(model.train(), batches, steps=6)
    assert not model.training and res["table"].shape == (2, 4, 6, 2) and res["count"].shape == (2, 3) and "table_all" not in res
    for b in range(2):
        _, sp = model.sparsification(left[b:b + 1], right[b:b + 1], gt[b:b + 1], steps=6)
        assert torch.equal(bits(res["table"][b]), bits(table_of(sp).cpu()[0])) and torch.equal(res["count"][b], sp.count.cpu()[0])
    want = res["table"].double().mean(0)
    assert torch.equal(res["dataset"]["epe"], want[:3, :, 0]) and torch.equal(res["dataset"]["oracle_d1"], want[3, :, 1])
    assert torch.equal(res["dataset"]["ause_epe"], (want[:3, :, 0] - want[3:, :, 0]).mean(1)) and res["dataset"]["samples"] == 2
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        res1 = D.evaluate_sparsification(model, batches, steps=6)
    finally:
        dist.destroy_process_group()
    assert torch.equal(bits(res1["table_all"]), bits(res["table"])) and torch.equal(res1["count_all"], res["count"])
    assert all(torch.equal(res1["dataset"][k], res["dataset"][k]) for k in ("epe", "d1", "oracle_epe", "ause_d1", "aurg_epe"))
    with pytest.raises(RuntimeError, match="no batches"):
        D.evaluate_sparsification(model, [])
    ecm.ops.check_async_errors()
