"""CPU-side contract of the opt-in split-bf16 products (ops.split_products, csrc/split_bf16.hip): the split itself in the kernel's
own bit operations, the packed-weight layout, the case table of tests/test_hip_split_bf16_fp64.py against the tile constants parsed
from the source, the C ABI entries and the switch.  No GPU needed."""
import os
import re

import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

CSRC = os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc")
SRC = os.path.join(CSRC, "split_bf16.hip")
BODY = os.path.join(CSRC, "bf16_conv3d.h")           # the implicit-GEMM body split_bf16.hip and bf16_infer.hip share
NEW_ENTRIES = ("ecm_conv3d_split_packed_elems", "ecm_conv3d_split_pack_weight", "ecm_conv3d_k3s2_split_fwd",
               "ecm_deconv3d_k3s2_split_fwd")

# ---- the tile constants, restated; test_constants_match_the_source pins them to split_bf16.hip (TW, NSLOT: bf16_conv3d.h) -------
TW, NSLOT, NTERM, CONV_SLOTS = 32, 28, 3, 27
S2_TD, S2_TH, DC_TD, DC_TH = 2, 2, 4, 4
LIMIT = 2.0 ** -110             # |x| >= LIMIT: x1 + x2 + x3 == x exactly (the header comment's guaranteed range)


def _src_const(name, path=SRC):
    m = re.search(r"\b%s = (\d+)" % name, open(path).read())
    assert m, name
    return int(m.group(1))


def test_constants_match_the_source():
    for name, val in (("TW", TW), ("NSLOT", NSLOT)):
        assert _src_const(name, BODY) == val, name
    for name, val in (("NTERM", NTERM), ("CONV_SLOTS", CONV_SLOTS), ("S2_TD", S2_TD), ("S2_TH", S2_TH), ("DC_TD", DC_TD), ("DC_TH", DC_TH)):
        assert _src_const(name) == val, name
    src = open(SRC).read()
    assert "2^-110" in src and "tests/test_split_bf16_cpu.py" in src      # the documented range, and the pointer to this restatement


def test_conv3d_body_exists_once():
    """The tap geometry, the staging, the MFMA block, the phase switch and the launch live in bf16_conv3d.h alone: the two kernel
    families built on it hold their operand policy, tile shapes and entries, and split3 is split_bf16.hip's."""
    body = open(BODY).read()
    users = [open(os.path.join(CSRC, f)).read() for f in ("bf16_infer.hip", "split_bf16.hip")]
    for u in users:
        assert '#include "bf16_conv3d.h"' in u
    for pattern in (r"constexpr int TW\b", r"constexpr int NSLOT\b", r"constexpr void dc_tap\(", r"struct Geo\b", r"constexpr int tap_off\(",
                    r"__builtin_amdgcn_make_buffer_rsrc\(", r"__builtin_amdgcn_mfma_f32_32x32x16_bf16\(", r"#define ECM_DC_PHASE\b",
                    r"ecm_allow_lds\(", r"hipLaunchKernelGGL\(\(conv3d_taps<"):
        assert len(re.findall(pattern, body)) == 1, pattern
    for name in ("dc_tap(", "struct Geo", "tap_off(", "make_buffer_rsrc(", "mfma_f32_32x32x16_bf16(", "ECM_DC_PHASE", "ecm_allow_lds(",
                 "hipLaunchKernelGGL", "__global__", "__syncthreads"):
        for u in users:
            assert name not in u, name
    assert "split3" not in body and "split3" not in users[0]
    assert len(re.findall(r"__device__ __forceinline__ void split3\(", users[1])) == 1


def test_lds_budget():
    """The budget of the header comment: three terms of halo + zero position + staged weight slots, 16 bytes each."""
    halo = lambda s, td, th, extra: (s * (td - 1) + 1 + extra) * (s * (th - 1) + 1 + extra) * (s * (TW - 1) + 1 + extra)   # noqa: E731
    conv = NTERM * (halo(2, S2_TD, S2_TH, 2) + 1 + CONV_SLOTS * 64) * 16
    dec = NTERM * (halo(1, DC_TD, DC_TH, 1) + 1 + 8 * 64) * 16
    assert conv <= 160 * 1024 and 2 * dec <= 160 * 1024, (conv, dec)


# ---- the split, in the kernel's bit operations (split3 of split_bf16.hip) ---------------------------------------------------------
def split3(x):
    """fp32 tensor -> three fp32 tensors holding bf16 values: truncate, subtract (exact), truncate, subtract, truncate."""
    u = x.view(torch.int32)
    top = lambda v: (v.view(torch.int32) & -65536).view(torch.float32)       # noqa: E731  (the top 16 bits)
    fin = torch.isfinite(x)
    x1 = top(x)
    r1 = x - x1
    x2 = top(r1)
    r2 = r1 - x2
    x3 = top(r2)
    nan = torch.isnan(x)
    x1 = torch.where(nan, ((u >> 16 | 0x40) << 16).view(torch.float32), x1)  # a NaN keeps a quiet bit
    zero = torch.zeros_like(x)
    return x1, torch.where(fin, x2, zero), torch.where(fin, x3, zero)


def _is_bf16(t):
    return bool(((t.view(torch.int32) & 0xffff) == 0).all())


def test_split_reproduces_every_fp32_value():
    g = torch.Generator().manual_seed(110)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 16,), generator=g, dtype=torch.int64).to(torch.int32)
    exps = torch.arange(1 << 16, dtype=torch.int32) % 255                    # every finite exponent field, 0 (subnormal) included
    bits = (bits & ~0x7f800000) | (exps << 23)
    x = bits.view(torch.float32)
    flt_max = torch.finfo(torch.float32).max
    special = torch.tensor([flt_max, -flt_max, 1 - 2.0 ** -24, 16777215.0, 0.0, -0.0, LIMIT, -LIMIT * (2 - 2.0 ** -23),
                            2.0 ** -126, 2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -127 + 2.0 ** -133], dtype=torch.float32)
    for t, exact_everywhere in ((x, False), (special, True)):
        x1, x2, x3 = split3(t)
        assert all(_is_bf16(v) for v in (x1, x2, x3))
        assert torch.isfinite(x1).all()                                       # truncation: FLT_MAX does not round up to Inf
        s = x1.double() + x2.double() + x3.double()
        err = (s - t.double()).abs()
        inside = (t.abs() >= LIMIT) | (t == 0) | exact_everywhere
        assert float(err[inside].max()) == 0.0
        assert float(err.max()) < 2.0 ** -133                                # below the range only bits under the smallest bf16 subnormal go
        assert bool(((x2 == 0) | (torch.sign(x2) == torch.sign(t))).all()) and bool(((x3 == 0) | (torch.sign(x3) == torch.sign(t))).all())
    assert int((x.abs() < LIMIT).sum()) > 1000 and int((x.abs() >= LIMIT).sum()) > 50000
    # the fp32 sum too (the order the accumulator sees is immaterial: every partial sum is representable)
    x1, x2, x3 = split3(special)
    assert torch.equal((x3 + x2) + x1, special)


def test_split_of_non_finite_values():
    inf, nan = float("inf"), float("nan")
    sneaky = torch.tensor([0x7f800001], dtype=torch.int32).view(torch.float32)   # a NaN whose payload sits in the low 16 bits
    t = torch.cat([torch.tensor([inf, -inf, nan]), sneaky])
    x1, x2, x3 = split3(t)
    assert torch.equal(x1[:2], t[:2]) and bool(torch.isnan(x1[2:]).all())
    assert _is_bf16(x1) and float(x2.abs().max()) == 0.0 and float(x3.abs().max()) == 0.0


def test_six_products_meet_the_single_product_bound():
    """The bound test 2a of the GPU file asserts, on the emulation: the six leading products of the split terms, accumulated in
    fp32, are within 2^-21 relative of x*w."""
    g = torch.Generator().manual_seed(21)
    x, w = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    xs, ws = split3(x), split3(w)
    acc = torch.zeros(4096)
    for i, j in ((0, 2), (2, 0), (1, 1), (1, 0), (0, 1), (0, 0)):            # (weight term, activation term), smallest first
        acc = acc + ws[i] * xs[j]
    rel = ((acc.double() - x.double() * w.double()).abs() / (x.double() * w.double()).abs()).max()
    assert float(rel) <= 2.0 ** -21, float(rel)


# ---- the packed-weight image ----------------------------------------------------------------------------------------------------
def dc_ntaps(p):
    return (1 + ((p >> 2) & 1)) * (1 + ((p >> 1) & 1)) * (1 + (p & 1))


def dc_base(p):
    return sum((dc_ntaps(q) + 1) & ~1 for q in range(p))


def dc_tap(p, t):
    """tap t of output phase p -> ((kd,kh,kw), (ed,eh,ew)): o = 2m + p takes k = 1 at m (p = 0), or k = 0 at m+1 and k = 2 at m."""
    pd = ((p >> 2) & 1, (p >> 1) & 1, p & 1)
    n = [1 + v for v in pd]
    idx = (t // (n[1] * n[2]), (t // n[2]) % n[1], t % n[2])
    k, e = [], []
    for d in range(3):
        if not pd[d]:
            k.append(1), e.append(0)
        elif idx[d] == 0:
            k.append(0), e.append(1)
        else:
            k.append(2), e.append(0)
    return tuple(k), tuple(e)


def packed_image(w, transposed):
    """[Ci/8][3 terms][28 slots][Co][8] as fp32 tensors holding the bf16 terms (ecm_conv3d_split_pack_weight, restated)."""
    Ci, Co = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    img = torch.zeros(Ci // 8, NSLOT, Co, 8)
    wv = w.reshape(w.shape[0], w.shape[1], 27)
    if not transposed:
        img[:, :27] = wv.permute(1, 2, 0).reshape(Ci // 8, 8, 27, Co).permute(0, 2, 3, 1)
    else:
        for p in range(8):
            for t in range(dc_ntaps(p)):
                k, _ = dc_tap(p, t)
                img[:, dc_base(p) + t] = wv[:, :, (k[0] * 3 + k[1]) * 3 + k[2]].reshape(Ci // 8, 8, Co).permute(0, 2, 1)
    return torch.stack(split3(img), 1)


def test_phases_fill_the_slots_and_cover_every_tap_once():
    assert dc_base(8) == NSLOT and CONV_SLOTS == 27
    seen = sorted(dc_tap(p, t)[0] for p in range(8) for t in range(dc_ntaps(p)))
    assert seen == sorted((a, b, c) for a in range(3) for b in range(3) for c in range(3))
    for p in range(8):                                                        # o = 2(m + e) + k - 1 has the phase's parity
        for t in range(dc_ntaps(p)):
            k, e = dc_tap(p, t)
            assert all((2 * ee + kk - 1) == pp for kk, ee, pp in zip(k, e, ((p >> 2) & 1, (p >> 1) & 1, p & 1)))


def test_packed_image_restatement():
    w = torch.randn(64, 32, 3, 3, 3, generator=torch.Generator().manual_seed(3))
    img = packed_image(w, False)
    assert img.shape == (4, NTERM, NSLOT, 64, 8)
    assert torch.equal(img.sum(1)[2, 13, 40, 5], w[40, 21, 1, 1, 1]) and float(img[:, :, 27].abs().max()) == 0.0
    imt = packed_image(w, True)                                               # read as ConvTranspose3d [Ci = 64, Co = 32]
    assert imt.shape == (8, NTERM, NSLOT, 32, 8)
    assert torch.equal(imt.sum(1)[3, 0, 7, 2], w[26, 7, 1, 1, 1])             # phase 0's only tap is the centre
    k, _ = dc_tap(7, 5)
    assert torch.equal(imt.sum(1)[0, dc_base(7) + 5, 31, 1], w[1, 31][k])


# ---- the case table of tests/test_hip_split_bf16_fp64.py --------------------------------------------------------------------------
# name -> (B, Ci, Co, input dims, output dims, via): "ops" = through ecm_amd.ops forward + backward (so a conv case also launches the
# transposed kernel for its data gradient, onto its input dims, and a deconv case the convolution kernel), "abi" = one launch
# below ops' autograd, at extents it cannot produce.
def _o(dims):
    return tuple((d - 1) // 2 + 1 for d in dims)


CONV_CASES = {
    "c_one_voxel": (1, 32, 64, (1, 1, 1), (1, 1, 1), "ops"),                  # all halo is padding
    "c_chunk_walk": (1, 64, 64, (2, 2, 2), (1, 1, 1), "ops"),                 # eight channel chunks
    "c_odd": (1, 32, 64, (5, 9, 35), (3, 5, 18), "ops"),                      # partial w tile; ragged in d and h; gx onto 2n-1 extents
    "c_batch_ragged_w": (2, 64, 64, (4, 8, 70), (2, 4, 35), "ops"),           # Wo = 35: a full w tile plus a ragged one, batch > 1
    "c_deconv_adjoint": (1, 32, 64, (3, 16, 64), (2, 8, 32), "abi"),          # a full w tile; a [Ci,Co,27] weight read as Conv3d's
    "c_co32": (1, 64, 32, (3, 4, 33), (2, 2, 17), "ops"),                     # one output-channel tile
}
DECONV_CASES = {
    "t_smallest": (1, 64, 64, (1, 1, 1), (2, 2, 2), "ops"),
    "t_smallest_2n1": (1, 64, 64, (1, 1, 1), (1, 1, 1), "abi"),
    "t_ragged": (1, 64, 32, (3, 5, 33), (6, 10, 66), "ops"),
    "t_ragged_2n1": (1, 64, 32, (3, 5, 33), (5, 9, 65), "abi"),
    "t_batch": (2, 64, 64, (2, 4, 32), (4, 8, 64), "ops"),
    "t_full_d": (1, 32, 64, (4, 5, 3), (8, 10, 6), "ops"),                    # a full tile along d
}


def launches():
    """(kernel, Ci, Co, tiled grid, output dims) of every split launch the table makes."""
    out = []
    for B, Ci, Co, dims, od, via in CONV_CASES.values():
        assert od == _o(dims)
        out.append(("conv", Ci, Co, od, od))
        if via == "ops":
            out.append(("deconv", Co, Ci, od, dims))                          # the data gradient
    for B, Ci, Co, dims, od, via in DECONV_CASES.values():
        assert all(2 * n - 1 <= o <= 2 * n for n, o in zip(dims, od))
        out.append(("deconv", Ci, Co, dims, od))
        if via == "ops":
            assert od == tuple(2 * n for n in dims)
            out.append(("conv", Co, Ci, dims, dims))                          # the data gradient: the conv kernel back onto dims
    return out


def missing_classes():
    L = launches()
    want = {}
    for kern, tile in (("conv", (S2_TD, S2_TH, TW)), ("deconv", (DC_TD, DC_TH, TW))):
        mine = [l for l in L if l[0] == kern]
        for tiles in (1, 2):
            want[f"{kern}: {tiles} output-channel tile(s)"] = any(l[2] == 32 * tiles for l in mine)
        want[f"{kern}: more than one channel chunk"] = any(l[1] > 8 for l in mine)
        for ci in (32, 64):
            want[f"{kern}: Ci = {ci}"] = any(l[1] == ci for l in mine)
        for i, n in enumerate("dhw"):
            want[f"{kern}: ragged in {n}"] = any(l[3][i] % tile[i] for l in mine)
            want[f"{kern}: a full tile in {n}"] = any(l[3][i] >= tile[i] for l in mine)
        want[f"{kern}: more than one workgroup"] = any(
            -(-l[3][0] // tile[0]) * -(-l[3][1] // tile[1]) * -(-l[3][2] // tile[2]) > 1 for l in mine)
    dec = [l for l in L if l[0] == "deconv"]
    for p in range(8):
        pd = ((p >> 2) & 1, (p >> 1) & 1, p & 1)
        # the phase writes something: along a dimension where it is odd, output 2m+1 < extent needs extent >= 2
        writes = lambda l: all(l[4][i] >= 1 + pd[i] for i in range(3))        # noqa: E731
        want[f"deconv: phase {p}, 2n extents"] = any(writes(l) and all(o == 2 * n for n, o in zip(l[3], l[4])) for l in dec)
        want[f"deconv: phase {p}, 2n-1 extents"] = any(writes(l) and all(o == 2 * n - 1 for n, o in zip(l[3], l[4])) for l in dec)
    want["deconv: 1x1x1 output (only phase 0 writes)"] = any(l[4] == (1, 1, 1) for l in dec)
    return sorted(k for k, ok in want.items() if not ok)


def test_case_table_covers_every_class():
    assert missing_classes() == []


def test_case_table_is_small():
    for B, Ci, Co, dims, od, _ in list(CONV_CASES.values()) + list(DECONV_CASES.values()):
        assert B * max(Ci, Co) * max(dims[0] * dims[1] * dims[2], od[0] * od[1] * od[2]) <= 1 << 20


# ---- the C ABI and the switch ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ecm():
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def lib_mod(ecm):
    if not os.path.exists(ecm._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm._lib


def test_new_entries_exported_and_prototyped(lib_mod):
    import ctypes
    lib = ctypes.CDLL(lib_mod.LIB_PATH)
    for n in NEW_ENTRIES:
        assert n in lib_mod.PROTOTYPES and hasattr(lib, n) and n in declared(), n
    assert lib_mod.query("ecm_abi_version") >= 7


def test_size_query_and_argument_checks(lib_mod):
    assert lib_mod.query("ecm_conv3d_split_packed_elems", 32, 64) == 4 * NTERM * NSLOT * 64 * 8
    assert lib_mod.query("ecm_conv3d_split_packed_elems", 12, 32) == 0
    lib = lib_mod.load()
    assert lib.ecm_conv3d_k3s2_split_fwd(None, None, None, 1, 32, 32, 4, 4, 4, None) == -1
    assert lib.ecm_deconv3d_k3s2_split_fwd(None, None, None, 1, 64, 32, 4, 4, 4, 8, 8, 8, None) == -1


def test_default_is_fp32(ecm):
    assert not ecm.ops.split_products_on() or os.environ.get("ECM_SPLIT_BF16") == "1"
    assert ecm.ops.SPLIT_DEFAULT_KINDS <= ecm.ops.SPLIT_ALL_KINDS == {"conv_fwd", "conv_dgrad", "deconv_fwd", "deconv_dgrad"}


def test_split_products_nests_and_restores(ecm):
    ops = ecm.ops
    base = ops.split_products_on()
    with ops.split_products("bf16x3"):
        assert ops.split_products_on()
        with ops.split_products("fp32"):
            assert not ops.split_products_on()
            with ops.split_products("bf16x3", kinds=("conv_fwd",)):
                assert ops.split_products_on() and ops._SPLIT_KINDS == {"conv_fwd"}
            assert not ops.split_products_on()
        assert ops.split_products_on() and ops._SPLIT_KINDS == ops.SPLIT_DEFAULT_KINDS
    assert ops.split_products_on() == base
    with pytest.raises(KeyError):
        with ops.split_products("bf16x3"):
            raise KeyError("boom")
    assert ops.split_products_on() == base


@pytest.mark.parametrize("bad", ["bf16", "bf16x2", "tf32", torch.bfloat16, None])
def test_split_products_rejects_unknown_names(ecm, bad):
    with pytest.raises(ValueError):
        with ecm.ops.split_products(bad):
            pass
    with pytest.raises(ValueError):
        with ecm.ops.split_products("bf16x3", kinds=("conv_wgrad",)):
            pass
    assert not ecm.ops.split_products_on() or os.environ.get("ECM_SPLIT_BF16") == "1"


def test_supported_shapes_rule(ecm):
    ok = ecm.ops.split_supported
    assert ok(32, 64, 48 * 144 * 240) and ok(64, 64, 24 * 72 * 120) and ok(64, 32, 48 * 144 * 240)
    assert not ok(16, 64, 8) and not ok(32, 48, 8) and not ok(64, 64, 1 << 23)
