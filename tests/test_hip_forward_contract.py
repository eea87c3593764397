"""Every forward-only op of ops.py held to one operand contract on the MI355X, driven by
tests/forward_contract_table.py: per row and shape the CLEAN result -- fresh contiguous 16-byte-aligned operands on the default
stream -- is computed once and held to the row's restatement by that op's existing rule; every variant must then reproduce the
clean result bit for bit (fp32 as int32, NaN meets NaN): strided views with poisoned slack, both plane forms, a stride-0 batch,
operands 4 bytes off a 16-byte boundary and masks at odd addresses, bool against uint8 masks, a side stream whose operands are
written on that stream, the batch against its images, operands unchanged by the call, recycled NaN memory inside guard bands, and
a second call.  Every call is an ordinary successful call or a Python-level refusal."""
import collections

import pytest
import torch

import forward_contract_table as FT
from test_hip_guard_bands import POISON, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(name, case) for name in sorted(FT.ROWS) for case in FT.ROWS[name].cases]
IDS = [f"{n}-{c}" for n, c in CASES]
_CLEAN = {}


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def on_device(row, a):
    """Fresh, contiguous, aligned device copies of the row's tensor operands; everything else as it is."""
    out = collections.OrderedDict((k, v.to(DEV) if k in row.roles else v) for k, v in a.items())
    assert all(out[k].is_contiguous() and out[k].data_ptr() % 16 == 0 for k in row.roles)
    return out


def fresh(row, a):
    """a, with the operands the op may change cloned (a volume that is integrated into)."""
    return collections.OrderedDict((k, v.clone() if k in row.inplace else v) for k, v in a.items())


def clean(ecm, name, case):
    """(CPU operands, device operands, clean outputs), computed once per row and shape and held to the row's restatement."""
    if (name, case) not in _CLEAN:
        row = FT.ROWS[name]
        cpu = row.operands(case)
        a = on_device(row, cpu)
        out = tuple(t.clone() for t in row.call(ecm.ops, fresh(row, a)))
        torch.cuda.synchronize()
        row.hold(ecm.ops, cpu, tuple(t.cpu() for t in out), a, out)
        _CLEAN[(name, case)] = (cpu, a, out)
    return _CLEAN[(name, case)]


def same(got, want, what):
    torch.cuda.synchronize()
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert FT.bits_equal(g, w), f"{what}: output {i} differs from the clean result"


def run(ecm, row, a, **replace):
    b = fresh(row, a)
    b.update(replace)
    return row.call(ecm.ops, b)


def bdim(t):
    return 1 if t.dim() == 5 else 0                                        # a head volume is [NH,B,D,h,w]


def report(name, case, variant, ran, exempt):
    print(f"FORWARD-CONTRACT {name} {case} {variant}: ran {ran or '-'}; exempt {exempt or '-'}")


def exempt_of(row, variant):
    return {k: v for k, v in row.exempt.items() if k.split(":")[0] == variant}


def int_view(t):
    """t as integers of its element size (torch.cat and torch.equal take every such dtype)."""
    return t if t.dtype == torch.bool else t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def refused(ecm, row, a, k, t):
    """A non-contiguous volume plane: RuntimeError before any launch, and both planes keep their bits."""
    b = fresh(row, a)
    b[k] = t
    before = {n: b[n].clone() for n in ("tsdf", "wsum")}
    with pytest.raises(RuntimeError, match="contiguous"):
        row.call(ecm.ops, b)
    torch.cuda.synchronize()
    for n in ("tsdf", "wsum"):
        assert FT.bits_equal(b[n].contiguous(), before[n].contiguous()), f"{n} changed under a refused call"


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_strided_views_both_forms_and_a_stride_zero_batch(ecm, name, case):
    row = FT.ROWS[name]
    if "strided" in row.exempt:
        return report(name, case, "strided", [], exempt_of(row, "strided"))
    _, a, want = clean(ecm, name, case)
    ran = []
    views = {k: FT.strided(a[k]) for k in row.roles}
    assert all(not v.is_contiguous() for v, _ in views.values())
    for k, role in row.roles.items():
        if role == "volume":
            refused(ecm, row, a, k, views[k][0])
            ran.append(k + " refused")
        else:
            same(run(ecm, row, a, **{k: views[k][0]}), want, f"{name} {case}: {k} strided")
            ran.append(k)
    others = {k: v for k, (v, _) in views.items() if row.roles[k] != "volume"}
    if len(others) > 1:
        same(run(ecm, row, a, **others), want, f"{name} {case}: all strided")
        ran.append("all")
    for k, (v, buf) in views.items():
        assert FT.slack_intact(a[k], buf), f"{name} {case}: the slack columns of {k} were written"
    forms = FT.four_dim_operands(name)
    if forms:
        same(run(ecm, row, a, **{k: FT.four_dim(a[k]) for k in forms}), want, f"{name} {case}: the other plane form")
        ran.append("forms " + "+".join(forms))
    batched = [k for k, r in row.roles.items() if r != "volume"]
    if batched:
        pairs = {k: FT.expanded(a[k], bdim(a[k])) for k in batched}
        assert all(v.stride(bdim(v)) == 0 for v, _ in pairs.values())
        twin = tuple(t.clone() for t in run(ecm, row, a, **{k: t for k, (_, t) in pairs.items()}))
        same(run(ecm, row, a, **{k: v for k, (v, _) in pairs.items()}), twin, f"{name} {case}: a batch made by expand")
        ran.append("expand")
    report(name, case, "strided", ran, exempt_of(row, "strided") | exempt_of(row, "four_dim"))


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_misaligned_operands(ecm, name, case):
    row = FT.ROWS[name]
    if "misaligned" in row.exempt:
        return report(name, case, "misaligned", [], exempt_of(row, "misaligned"))
    _, a, want = clean(ecm, name, case)
    off = {k: FT.misaligned(a[k]) for k in row.roles}
    for k, t in off.items():
        assert t.is_contiguous() and (t.data_ptr() % 16 == 4 if t.element_size() == 4 else t.data_ptr() % 4 == 1), k
    ran = []
    for k in row.roles:                                                    # each alone (tsdf alone, wsum alone), then all together
        b = fresh(row, a)
        b[k] = FT.misaligned(a[k]) if k in row.inplace else off[k]
        same(row.call(ecm.ops, b), want, f"{name} {case}: {k} misaligned")
        ran.append(k)
    if len(off) > 1:
        b = fresh(row, a)
        b.update({k: FT.misaligned(a[k]) for k in row.roles})
        same(row.call(ecm.ops, b), want, f"{name} {case}: all misaligned")
        ran.append("all")
    report(name, case, "misaligned", ran, {})


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_mask_forms(ecm, name, case):
    row = FT.ROWS[name]
    masks = [k for k, r in row.roles.items() if r == "mask"]
    if not masks:
        return report(name, case, "mask_forms", [], exempt_of(row, "mask_forms"))
    _, a, want = clean(ecm, name, case)
    ran = []
    for k in masks:
        assert a[k].dtype == torch.bool
        for form, m in FT.mask_forms(a[k], row.masks.get(k, False)).items():
            same(run(ecm, row, a, **{k: m}), want, f"{name} {case}: {k} as {form}")
            ran.append(f"{k} {form}")
    report(name, case, "mask_forms", ran, {})


@pytest.fixture(scope="module")
def busy():
    """Device work of a few milliseconds: a 4096^2 fp32 matmul into a scratch tensor."""
    x = torch.randn(4096, 4096, device=DEV)
    out = torch.empty_like(x)
    return lambda: torch.matmul(x, x, out=out)


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_side_stream(ecm, busy, name, case):
    row = FT.ROWS[name]
    _, a, want = clean(ecm, name, case)
    b = fresh(row, a)
    truth = {k: b[k] for k in row.roles}
    for k, t in truth.items():                                             # buffers that hold poison until the side stream writes them
        b[k] = torch.full_like(t, FT.poison_of(t) if t.dtype != torch.bool else False)
        if t.dtype == torch.uint8:
            b[k].fill_(0 if row.roles[k] == "mask" else 255)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream() == s
        busy()
        for k, t in truth.items():
            b[k].copy_(t, non_blocking=True)
        got = row.call(ecm.ops, b)
        s.synchronize()
    same(got, want, f"{name} {case}: on a side stream")
    report(name, case, "side_stream", list(row.roles) or ["no tensor operand: the launch and the parameter copy alone"], {})


def image(row, a, b):
    """The operands of image b alone: every batched tensor's slice, every per-image matrix's row."""
    out = fresh(row, a) if not row.sequential else collections.OrderedDict(a)
    for k, r in row.roles.items():
        if r != "volume":
            out[k] = a[k].narrow(bdim(a[k]), b, 1).contiguous()
    for k in row.matrices:
        if a[k].dim() == 3:
            out[k] = a[k][b]
    return out


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_a_batch_is_its_images(ecm, name, case):
    row = FT.ROWS[name]
    if "batch" in row.exempt:
        return report(name, case, "batch", [], exempt_of(row, "batch"))
    _, a, want = clean(ecm, name, case)
    n = FT.B
    if row.sequential:                                                     # the views of one call are calls in order, into one volume
        vol = fresh(row, a)
        for b in range(n):
            got = row.call(ecm.ops, image(row, vol, b))
        same(got, want, f"{name} {case}: the views one by one")
        return report(name, case, "batch", ["views in order"], {})
    per = [tuple(t.clone() for t in row.call(ecm.ops, image(row, a, b))) for b in range(n)]
    ran = []
    for i, dim in enumerate(row.batch):
        if dim is not None:
            same((torch.cat([int_view(p[i]) for p in per], dim),), (int_view(want[i]),), f"{name} {case}: output {i} against its images")
            ran.append(f"output {i}")
    report(name, case, "batch", ran, exempt_of(row, "batch"))


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_inputs_are_untouched(ecm, name, case):
    row = FT.ROWS[name]
    if "untouched" in row.exempt:
        return report(name, case, "untouched", [], exempt_of(row, "untouched"))
    _, a, want = clean(ecm, name, case)
    b = fresh(row, a)
    before = {k: b[k].clone() for k in row.roles if k not in row.inplace}
    same(row.call(ecm.ops, b), want, f"{name} {case}: again")
    for k, t in before.items():
        assert FT.bits_equal(b[k], t), f"{name} {case}: {k} was written"
    report(name, case, "untouched", list(before), {k: "the op's stated in-place operand" for k in row.inplace})


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_recycled_memory_and_guard_bands(ecm, name, case):
    row = FT.ROWS[name]
    _, a, want = clean(ecm, name, case)
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 6, 1 << 10, 1 << 14, 1 << 17, 1 << 19, 1 << 21) for _ in range(4)]
    torch.cuda.synchronize()
    del junk                                                               # the allocator's free blocks now hold NaN ...
    same(row.call(ecm.ops, fresh(row, a)), want, f"{name} {case}: on recycled memory")        # ... and outputs and scratch come from them
    b = fresh(row, a)
    with guarded(ecm) as g:                                                # separately: the guard bands (their fill is 0xA5, not NaN)
        for k in row.inplace:                                              # a volume that is written lies between guard bands too
            t = ecm.ops.torch.empty(tuple(b[k].shape), dtype=b[k].dtype, device=DEV)
            t.copy_(b[k])
            b[k] = t
        got = row.call(ecm.ops, b)
        g.check(f"{name} {case}")
    assert POISON == 0xA5
    same(got, want, f"{name} {case}: inside guard bands")
    report(name, case, "recycled", [f"{len(g.records)} guarded allocations"], {})


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_twice(ecm, name, case):
    row = FT.ROWS[name]
    cpu, _, want = clean(ecm, name, case)
    same(row.call(ecm.ops, fresh(row, on_device(row, cpu))), want, f"{name} {case}: a second clean call")
    ecm.ops.check_async_errors()
    report(name, case, "twice", ["all operands fresh"], {})
