"""The speckle filter, the part that needs no GPU: `speckle_t` below, a sequential two-pass union-find in
numpy and plain Python that restates the definitions -- the reference of tests/test_hip_disp_speckle.py -- checked against closed
forms; the ABI addition; and the refusals of ops.disparity_speckle and _ECMNet.despeckle that come before any device work.

Definitions.  A pixel is usable iff d is finite and valid != 0 (valid None: all ones).  Two usable pixels of the same image are
connected iff they are 4-neighbours (no diagonals, no wrap from a row to the next or from an image to the next) and
|d[p] - d[q]| <= max_diff, in fp32 and inclusive.  A segment is a connected component of that graph.  label[p] is the row-major
index y*W + x, within its image, of the segment's first pixel, -1 where p is not usable; size[p] the segment's pixel count, 0
where p is not usable; out[p] is d[p], bit for bit, where p is usable and size[p] > max_size, else 0."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

INF, NAN = float("inf"), float("nan")


def kernel_constants():
    """The namespace-level constexpr ints of csrc/disp_speckle.hip by name (the GPU test places its shapes at the tile edges)."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "disp_speckle.hip")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr):
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


KC = kernel_constants()


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def segments_t(d, valid, max_diff):
    """(label, size) of d [B,H,W] as int32 arrays.  Pass one, row-major: a usable pixel is united with its left and its upper
    neighbour where connected (union by smaller index, so a root is the first pixel of its set).  Pass two: every pixel to its root,
    and the roots' counts."""
    d = np.ascontiguousarray(np.asarray(d, dtype=np.float32))
    B, H, W = d.shape
    ok = np.isfinite(d)
    if valid is not None:
        ok &= np.asarray(valid).reshape(B, H, W) != 0
    tol = np.float32(max_diff)
    with np.errstate(invalid="ignore", over="ignore"):                 # inf - inf and overflow at pixels that `ok` masks, or compare false
        left = np.zeros((B, H, W), dtype=bool)
        left[:, :, 1:] = ok[:, :, 1:] & ok[:, :, :-1] & (np.abs(d[:, :, 1:] - d[:, :, :-1]) <= tol)
        up = np.zeros((B, H, W), dtype=bool)
        up[:, 1:] = ok[:, 1:] & ok[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= tol)
    label, size = np.full((B, H * W), -1, dtype=np.int32), np.zeros((B, H * W), dtype=np.int32)
    for b in range(B):
        parent = list(range(H * W))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        usable, lf, uf = ok[b].ravel().tolist(), left[b].ravel().tolist(), up[b].ravel().tolist()
        for i in range(H * W):
            for joined, j in ((lf[i], i - 1), (uf[i], i - W)):
                if joined:
                    a, c = find(i), find(j)
                    if a != c:
                        parent[max(a, c)] = min(a, c)
        roots = [find(i) if usable[i] else -1 for i in range(H * W)]
        label[b] = roots
        counts = np.bincount(np.asarray([r for r in roots if r >= 0], dtype=np.int64), minlength=H * W)
        size[b] = np.where(label[b] >= 0, counts[np.maximum(label[b], 0)], 0)
    return label.reshape(B, H, W), size.reshape(B, H, W)


def removed_t(d, size, max_size):
    """out of the definition, from the size plane."""
    d = np.asarray(d, dtype=np.float32)
    return np.where(size > max_size, d, np.float32(0))


def speckle_t(d, valid, max_size, max_diff):
    """(out, label, size) as torch tensors: float32, int32, int32."""
    label, size = segments_t(d, valid, max_diff)
    return torch.from_numpy(removed_t(d, size, max_size)), torch.from_numpy(label), torch.from_numpy(size)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_a_constant_plane_is_one_segment():
    d = torch.full((1, 5, 7), 3.5)
    out, label, size = speckle_t(d, None, 34, 0.0)
    assert bool((label == 0).all()) and bool((size == 35).all()) and same_bits(out, d)
    assert bool((speckle_t(d, None, 35, 0.0)[0] == 0).all())


def test_a_checkerboard_is_all_singletons():
    y, x = torch.arange(6).view(6, 1), torch.arange(9).view(1, 9)
    d = ((y + x) % 2).float().view(1, 6, 9) * 1.5 + 1
    out, label, size = speckle_t(d, None, 0, 1.0)
    assert bool((size == 1).all()) and torch.equal(label.view(-1), torch.arange(54, dtype=torch.int32)) and same_bits(out, d)
    assert bool((speckle_t(d, None, 1, 1.0)[0] == 0).all())


def test_the_comparison_is_inclusive_and_not_transitive():
    H, W = 4, 12
    ramp = (torch.arange(W).float() * 0.25).view(1, 1, W).expand(1, H, W).contiguous()
    _, label, size = speckle_t(ramp, None, 0, 0.25)                    # step == max_diff: one segment, ends 2.75 apart
    assert bool((label == 0).all()) and bool((size == H * W).all())
    below = float(np.nextafter(np.float32(0.25), np.float32(0)))       # the steps of 0.25 are exact in fp32; max_diff one ulp under them
    assert below < 0.25 and math.isclose(below, 0.25, rel_tol=1e-6)
    _, label, size = speckle_t(ramp, None, 0, below)                   # step just above max_diff: W columns of H pixels
    assert bool((size == H).all()) and torch.equal(label, torch.arange(W, dtype=torch.int32).view(1, 1, W).expand(1, H, W))


def test_diagonal_neighbours_are_not_connected():
    d = torch.full((1, 4, 4), 9.0)
    d[0, :2, :2] = 1.0
    d[0, 2:, 2:] = 1.0
    _, label, size = speckle_t(d, None, 0, 0.5)
    assert int(label[0, 1, 1]) == 0 and int(label[0, 2, 2]) == 10 and int(size[0, 1, 1]) == 4 and int(size[0, 2, 2]) == 4
    assert int(label[0, 0, 2]) == 2 and int(label[0, 2, 0]) == 8      # the 9s meet only diagonally too


@pytest.mark.parametrize("k", [1, 5, 6])
def test_a_blob_of_max_size_is_removed_and_one_pixel_more_is_kept(k):
    d = torch.full((1, 5, 8), 2.0)
    blob = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4)][:k]
    for y, x in blob:
        d[0, y, x] = 7.0
    out, _, size = speckle_t(d, None, k, 1.0)
    assert all(int(size[0, y, x]) == k and float(out[0, y, x]) == 0 for y, x in blob) and int((out == 0).sum()) == k
    out = speckle_t(d, None, k - 1, 1.0)[0]
    assert same_bits(out, d)


def test_nothing_usable():
    d = torch.rand(2, 3, 4)
    for dd, valid in ((d, torch.zeros(2, 3, 4, dtype=torch.uint8)), (torch.full((2, 3, 4), NAN), None)):
        out, label, size = speckle_t(dd, valid, 0, 1.0)
        assert bool((label == -1).all()) and bool((size == 0).all()) and bool((out == 0).all())


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_non_finite_values_are_unusable_and_separate_their_neighbours(bad):
    d = torch.full((1, 3, 7), 1.0)
    d[0, :, 3] = bad
    out, label, size = speckle_t(d, None, 0, 1.0)
    assert bool((label[0, :, 3] == -1).all()) and bool((size[0, :, 3] == 0).all()) and bool((out[0, :, 3] == 0).all())
    assert bool((label[0, :, :3] == 0).all()) and bool((label[0, :, 4:] == 4).all()) and bool((size[0, :, :3] == 9).all())
    assert bool(torch.isfinite(out).all())


def test_an_invalid_column_separates_the_plane():
    d = torch.full((1, 4, 9), 5.0)
    valid = torch.ones(1, 4, 9, dtype=torch.uint8)
    valid[0, :, 2] = 0
    _, label, size = speckle_t(d, valid, 0, 0.0)
    assert bool((label[0, :, :2] == 0).all()) and bool((size[0, :, :2] == 8).all())
    assert bool((label[0, :, 3:] == 3).all()) and bool((size[0, :, 3:] == 24).all()) and bool((label[0, :, 2] == -1).all())


def test_rows_and_images_do_not_wrap():
    # the last pixel of a row and the first of the next hold the same value, and nothing else joins them
    d = torch.tensor([[[1.0, 5.0, 9.0, 2.0], [2.0, 6.0, 10.0, 14.0]]])
    _, label, size = speckle_t(d, None, 0, 0.5)
    assert bool((size == 1).all()) and int(label[0, 0, 3]) == 3 and int(label[0, 1, 0]) == 4
    # two images of one constant: two segments, each labelled inside its own image
    d = torch.full((2, 3, 3), 1.0)
    _, label, size = speckle_t(d, None, 0, 0.5)
    assert bool((label == 0).all()) and bool((size == 9).all())


def test_negative_zero_and_bits_pass_through():
    d = torch.tensor([[[-0.0, 0.0, 1e-40, 3.0]]])
    out, label, size = speckle_t(d, None, 0, 1.0)
    assert same_bits(out, d) and label.view(-1).tolist() == [0, 0, 0, 3] and size.view(-1).tolist() == [3, 3, 3, 1]


def test_speckle_t_agrees_with_a_flood_fill():
    g = torch.Generator().manual_seed(3)
    d = torch.randint(0, 16, (2, 9, 11), generator=g).float() / 4
    valid = torch.rand(2, 9, 11, generator=g) >= 0.3
    for tol in (0.0, 0.25, 1.0):
        _, label, size = speckle_t(d, valid, 0, tol)
        B, H, W = d.shape
        seen = torch.full((B, H, W), -1, dtype=torch.int32)
        for b in range(B):
            for s in range(H * W):
                if not valid[b, s // W, s % W] or seen[b, s // W, s % W] >= 0:
                    continue
                stack, members = [s], []
                seen[b, s // W, s % W] = s
                while stack:
                    p = stack.pop()
                    members.append(p)
                    y, x = p // W, p % W
                    for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                        if 0 <= yy < H and 0 <= xx < W and valid[b, yy, xx] and seen[b, yy, xx] < 0 \
                                and abs(float(d[b, y, x]) - float(d[b, yy, xx])) <= tol:
                            seen[b, yy, xx] = s
                            stack.append(yy * W + xx)
                for p in members:
                    assert int(size[b, p // W, p % W]) == len(members)
        assert torch.equal(seen, label)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_mod():
    import ecm_amd
    if not os.path.exists(ecm_amd._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm_amd._lib


def test_header_and_prototypes_hold_the_new_entry(lib_mod):
    assert "ecm_disp_speckle_fwd" in declared() and "ecm_disp_speckle_fwd" in lib_mod.PROTOTYPES
    assert lib_mod.missing_symbols() == []
    assert lib_mod.query("ecm_abi_version") >= 12
    assert len(lib_mod.PROTOTYPES["ecm_disp_speckle_fwd"][1]) == 10
    assert KC["TW"] == KC["WAVE"] == 64 and KC["THREADS"] == 256 and KC["TH"] % KC["NWAVE"] == 0 and KC["TH"] >= 2


def test_bad_arguments_are_rejected_without_touching_the_gpu(lib_mod):
    import ctypes as C
    f = lib_mod.load().ecm_disp_speckle_fwd
    p = C.c_void_p(64)                                                 # never dereferenced: every call below returns first
    assert f(None, None, None, None, 1, 1, 1, 0, 0.0, None) == -1
    assert f(None, p, p, p, 1, 4, 4, 1, 1.0, None) == -1 and f(p, p, None, p, 1, 4, 4, 1, 1.0, None) == -1
    assert f(p, p, p, None, 1, 4, 4, 1, 1.0, None) == -1
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert f(p, None, p, p, B, H, W, 1, 1.0, None) == -1
    for max_size in (-1, -(1 << 31)):
        assert f(p, None, p, p, 1, 4, 4, max_size, 1.0, None) == -1
    for max_diff in (-1.0, -1e-30, NAN, INF, -INF):
        assert f(p, None, p, p, 1, 4, 4, 1, max_diff, None) == -1
    assert f(p, None, p, p, 1 << 11, 1 << 10, 1 << 10, 1, 1.0, None) == -2             # B H W = 2^31


# ---- the refusals that come before any device work: all of this runs on CPU tensors -------------------------------------------------
def test_check_speckle_parameters():
    import ecm_amd
    ops = ecm_amd.ops
    got = ops.check_speckle_parameters(np.int64(7), 1)
    assert got == (7, 1.0) and type(got[0]) is int and type(got[1]) is float
    assert ops.check_speckle_parameters(0, 0.0) == (0, 0.0)
    for bad in (True, False, -1, 2.0, None, "3"):
        with pytest.raises(ValueError, match="max_size"):
            ops.check_speckle_parameters(bad, 1.0)
    for bad in (NAN, INF, -INF, -0.5, True, None, "1"):
        with pytest.raises(ValueError, match="max_diff"):
            ops.check_speckle_parameters(5, bad)
    with pytest.raises(ValueError, match="^despeckle: "):
        ops.check_speckle_parameters(-1, 1.0, "despeckle")


def test_op_refusals():
    import ecm_amd
    ops = ecm_amd.ops
    d = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.disparity_speckle(d)
    with pytest.raises(ValueError, match="max_size"):                  # before the tensor is looked at
        ops.disparity_speckle(d, max_size=-1)
    with pytest.raises(ValueError, match="max_diff"):
        ops.disparity_speckle(d, max_diff=NAN)
    sig = inspect.signature(ops.disparity_speckle)
    assert list(sig.parameters) == ["disp", "valid", "max_size", "max_diff", "with_segments"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 200, 1.0, False]


def test_refine_keeps_its_signature_and_despeckle_appends_two_keywords():
    import ecm_amd
    from ecm_amd import models
    assert models.Despeckled._fields == models.Refined._fields + ("despeckled", "segment")
    assert models.Refined._fields == models.CrossCheck._fields + ("median", "refined")
    today = ["self", "left", "right", "threshold", "rel", "head", "median_radius", "bilateral_radius", "sigma_space", "sigma_color"]
    defaults = [1.0, 0.0, 2, 2, 4, 2.0, 0.25]
    sig = inspect.signature(models._ECMNet.refine)
    assert list(sig.parameters) == today and [p.default for p in list(sig.parameters.values())[3:]] == defaults
    sig = inspect.signature(models._ECMNet.despeckle)
    assert list(sig.parameters) == today + ["speckle_size", "speckle_diff"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == defaults + [200, 1.0]
    assert list(inspect.signature(models._ECMNet.cross_check).parameters) == today[:6]
    x = torch.zeros(1, 3, 64, 128)
    net = ecm_amd.get_model("cmfsm")
    for kw, what in (({"speckle_size": -1}, "max_size"), ({"speckle_size": 2.0}, "max_size"), ({"speckle_size": True}, "max_size"),
                     ({"speckle_diff": -1.0}, "max_diff"), ({"speckle_diff": NAN}, "max_diff"), ({"head": 3}, "head"),
                     ({"median_radius": 4}, "radius"), ({"sigma_color": 0.0}, "sigma_color")):
        with pytest.raises(ValueError, match=what):
            net.despeckle(x, x, **kw)
    with pytest.raises(RuntimeError):                                  # speckle_diff is not looked at while speckle_size is None
        net.despeckle(x, x, speckle_size=None, speckle_diff=NAN)
    with pytest.raises(RuntimeError):
        net.despeckle(x, x, speckle_size=50)
    assert all(hasattr(cls, "despeckle") and hasattr(cls, "refine") for cls in models._MODELS.values())
