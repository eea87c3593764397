"""Disparity reprojection, the part that needs no GPU: `reproject_t` and `cloud_t` below, fp64 torch
restatements of the definition in include/ecm_geometry.h -- the reference of tests/test_hip_disp_reproject.py -- checked against
closed forms and at the edges of the predicate; then the signatures of the second ABI table's entries (ENTRIES below; the census
of _lib.GEOMETRY_PROTOTYPES against include/ecm_geometry.h is tests/test_abi_types.py's) and the refusals of ops.q_matrix,
ops.disparity_reproject, ops.point_cloud and _ECMNet.point_cloud that come before any device work.

Definition.  For pixel (x, y) of image b with disparity d: row r of Q_b [x y d 1]^T is ((Q[r][0] x + Q[r][1] y) + Q[r][2] d) + Q[r][3],
every operation one fp64 operation; the point is (X/W, Y/W, Z/W), each rounded once to fp32.  Usable: d finite, valid != 0,
min_disp < d <= max_disp in fp32, W finite and non-zero.  Unusable pixels are +0.0 in the dense planes; the cloud is the usable
pixels in row-major order, image after image."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from test_abi_types import PACKAGE, header_prototypes, lib_mod  # noqa: F401  (lib_mod: a fixture)

ENTRIES = ("ecmg_point_cloud_fwd", "ecmg_point_cloud_scratch_bytes", "ecmg_point_cloud_tile", "ecmg_reproject_fwd")
NAN, INF = float("nan"), float("inf")
FLT_MAX = 3.4028234663852886e38


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def reproject_t(d, Q, valid=None, min_disp=0.0, max_disp=None):
    """(xyz [B,3,H,W] fp32, mask [B,H,W] bool, xyz64 [B,3,H,W] fp64 before the rounding) of d [B,H,W] fp32 and Q [4,4] or [B,4,4]."""
    assert d.dtype == torch.float32 and d.dim() == 3
    B, H, W = d.shape
    q = Q.to(torch.float64).expand(B, 4, 4)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    dd = d.to(torch.float64)

    def row(r):
        e = lambda c: q[:, r, c].view(B, 1, 1)                                                   # noqa: E731
        return ((e(0) * x + e(1) * y) + e(2) * dd) + e(3)

    w = row(3)
    lo = torch.tensor(min_disp, dtype=torch.float32)
    hi = torch.tensor(FLT_MAX if max_disp is None else max_disp, dtype=torch.float32)
    mask = torch.isfinite(d) & (d > lo) & (d <= hi) & torch.isfinite(w) & (w != 0)
    if valid is not None:
        mask = mask & (valid != 0)
    xyz64 = torch.stack([row(0) / w, row(1) / w, row(2) / w], 1)
    xyz64 = torch.where(mask.unsqueeze(1), xyz64, torch.zeros_like(xyz64))
    return xyz64.to(torch.float32), mask, xyz64


def cloud_t(d, Q, attributes=None, valid=None, min_disp=0.0, max_disp=None):
    """(points [N, 3 + C] fp32, offsets [B + 1] int64, xyz, mask, points64 [N, 3]): the usable pixels by nonzero, row-major."""
    xyz, mask, xyz64 = reproject_t(d, Q, valid, min_disp, max_disp)
    b, y, x = mask.nonzero(as_tuple=True)                                                         # sorted: (b, y, x) ascending
    cols = [xyz[b, :, y, x]]
    if attributes is not None and attributes.shape[1]:
        cols.append(attributes[b, :, y, x])
    counts = mask.flatten(1).sum(1)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    return torch.cat(cols, 1), offsets, xyz, mask, xyz64[b, :, y, x]


def kernel_constants():
    """The constexpr ints of csrc/disp_geom.h by name."""
    src = open(os.path.join(PACKAGE, "csrc", "disp_geom.h")).read()
    env = {}
    for stmt in re.findall(r"^constexpr int ([^;]+);", src, flags=re.M):
        for name, expr in re.findall(r"(\w+) = ([^,]+)", stmt):
            if re.fullmatch(r"[\w\s*/+-]+", expr):
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


def well_conditioned(Q, H, W):
    """The condition under which a device fp64 evaluation lands within one fp32 ulp of reproject_t (the GPU file asserts it on its
    fixtures): q_matrix's form with Q30 = Q31 = 0, Q32 > 0 and Q33 >= 0 -- so, for d > 0, Q32 d and Q33 have one sign and W does not
    cancel -- and every |x - cx|, |y - cy| at least 2^-10, so that no coordinate comes near a zero crossing."""
    q = Q.to(torch.float64).reshape(-1, 4, 4)
    form = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.float64)
    free = torch.tensor([[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 1, 1]], dtype=torch.bool)
    ok = bool((q[:, ~free] == form[~free]).all()) and bool((q[:, 3, 2] > 0).all()) and bool((q[:, 3, 3] >= 0).all())
    x, y = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    ok = ok and bool(((x.view(1, -1) + q[:, 0, 3:4]).abs() >= 2.0 ** -10).all())
    return ok and bool(((y.view(1, -1) + q[:, 1, 3:4]).abs() >= 2.0 ** -10).all())


def ecm():
    import ecm_amd
    return ecm_amd


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_q_matrix_rows():
    Q = ecm().ops.q_matrix(700.0, 0.25, 320.5, 240.25, cx_right=322.5, x0=16, y0=8)
    assert Q.dtype == torch.float64 and Q.shape == (4, 4) and not Q.is_cuda
    assert Q.tolist() == [[1, 0, 0, -(320.5 - 16)], [0, 1, 0, -(240.25 - 8)], [0, 0, 0, 700.0], [0, 0, 4.0, -(320.5 - 322.5) / 0.25]]
    Q = ecm().ops.q_matrix(700.0, 0.25, 320.5, 240.25)
    assert Q[3, 3].item() == 0.0 and not torch.signbit(Q[3, 3])                       # +0.0: W's zero test is on the value anyway


def test_depth_and_lateral_closed_forms():
    f, b, cx, cy = 512.0, 0.5, 3.5, 1.25                                               # powers of two and short fractions: exact
    Q = ecm().ops.q_matrix(f, b, cx, cy)
    d = torch.tensor([[[1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 0.5]] * 3])
    xyz, mask, _ = reproject_t(d, Q)
    assert bool(mask.all())
    x = torch.arange(8.0).view(1, 1, 8).expand(1, 3, 8)
    y = torch.arange(3.0).view(1, 3, 1).expand(1, 3, 8)
    Z = f * b / d
    assert torch.equal(xyz[:, 2], Z)
    assert torch.equal(xyz[:, 0], (x - cx) * Z / f) and torch.equal(xyz[:, 1], (y - cy) * Z / f)


def test_crop_origin_shifts_x_and_y_only_and_cx_right_shifts_d():
    ops = ecm().ops
    f, b, cx, cy = 512.0, 0.5, 35.5, 17.25
    d = torch.tensor([[[1.0, 2.0, 4.0, 8.0]] * 2])
    base = reproject_t(d, ops.q_matrix(f, b, cx, cy))[0]
    crop = reproject_t(d, ops.q_matrix(f, b, cx, cy, x0=32, y0=16))[0]
    Z = f * b / d
    assert torch.equal(crop[:, 2], base[:, 2])
    assert torch.equal(crop[:, 0] - base[:, 0], 32 * Z / f) and torch.equal(crop[:, 1] - base[:, 1], 16 * Z / f)
    shifted = reproject_t(d + 0.5, ops.q_matrix(f, b, cx, cy, cx_right=cx - 0.5))[0]     # Z = f b / (d - (cx - cx_right))
    assert torch.equal(shifted, base)


def test_per_image_matrices_and_the_cloud_order():
    ops = ecm().ops
    Q = torch.stack([ops.q_matrix(512.0, 0.5, 3.5, 1.25), ops.q_matrix(256.0, 1.0, 2.5, 0.75)])
    d = torch.full((2, 2, 5), 2.0)
    valid = torch.tensor([[[1, 0, 1, 0, 0], [0, 0, 0, 0, 1]], [[0, 0, 0, 0, 0], [0, 1, 1, 0, 0]]], dtype=torch.uint8)
    index = torch.arange(20, dtype=torch.float32).view(2, 1, 2, 5)
    points, offsets, xyz, mask, _ = cloud_t(d, Q, index, valid)
    assert offsets.tolist() == [0, 3, 5] and points.shape == (5, 4)
    assert points[:, 3].tolist() == [0, 2, 9, 16, 17]                                   # row-major, image after image
    assert points[:, 2].tolist() == [128.0] * 3 + [128.0] * 2 and points[3, 0].item() == (1 - 2.5) * 128.0 / 256.0
    assert torch.equal(mask, valid.bool()) and bool((xyz[~mask.unsqueeze(1).expand(-1, 3, -1, -1)] == 0).all())
    one = [cloud_t(d[i:i + 1], Q[i], index[i:i + 1], valid[i:i + 1])[0] for i in range(2)]
    assert torch.equal(torch.cat(one), points)                                          # an image's rows do not depend on the batch
    empty = cloud_t(d, Q, index, torch.zeros_like(valid))
    assert empty[0].shape == (0, 4) and empty[1].tolist() == [0, 0, 0]


# ---- the edges of the predicate -------------------------------------------------------------------------------------------------------
def test_bounds_are_exclusive_below_and_inclusive_above():
    Q = ecm().ops.q_matrix(100.0, 1.0, 0.5, 0.5)
    below, above = 1.9999999, 8.000001                                                  # the fp32 neighbours of 2 and 8
    d = torch.tensor([[[below, 2.0, 2.0000002, 7.9999995, 8.0, above]]])
    assert reproject_t(d, Q, None, 2.0, 8.0)[1].tolist() == [[[False, False, True, True, True, False]]]
    assert reproject_t(d, Q, None, 2.0, None)[1].tolist() == [[[False, False, True, True, True, True]]]
    assert reproject_t(d, Q, None, 2.0, INF)[1].tolist() == [[[False, False, True, True, True, True]]]
    # the bound is rounded to fp32 like the map: 2 + 2^-30 is 2.0 there, and d == 2.0 stays out
    assert reproject_t(d, Q, None, 2.0 + 2.0 ** -30, None)[1].tolist() == [[[False, False, True, True, True, True]]]
    assert reproject_t(torch.tensor([[[0.0, -0.0, 1e-45]]]), Q)[1].tolist() == [[[False, False, True]]]   # the default: d > 0


def test_non_finite_disparities_and_the_valid_plane():
    Q = ecm().ops.q_matrix(100.0, 1.0, 0.5, 0.5)
    d = torch.tensor([[[NAN, INF, -INF, 4.0, 4.0, 4.0]]])
    valid = torch.tensor([[[1, 1, 1, 0, 1, 255]]], dtype=torch.uint8)
    xyz, mask, _ = reproject_t(d, Q, valid, -1.0, None)
    assert mask.tolist() == [[[False, False, False, False, True, True]]]
    assert bool(torch.isfinite(xyz).all()) and bool((xyz[0, :, 0, :4].view(torch.int32) == 0).all())     # +0.0, bit for bit
    assert xyz[0, 2, 0, 4].item() == 25.0


def test_a_zero_w_is_dropped():
    Q = ecm().ops.q_matrix(100.0, 1.0, 0.5, 0.5)
    assert Q[3, 0] == 0 and Q[3, 1] == 0 and Q[3, 3] == 0
    d = torch.tensor([[[-0.0, 0.0, -0.5, 0.5]]])
    xyz, mask, _ = reproject_t(d, Q, None, -1.0, None)                                   # W = Q32 d: exactly 0 at both zeros
    assert mask.tolist() == [[[False, False, True, True]]]
    assert bool((xyz[0, :, 0, :2].view(torch.int32) == 0).all()) and xyz[0, 2, 0, 2].item() == -200.0
    Qinf = Q.clone()
    Qinf[3, 2] = 1e308                                                                   # W overflows for d = 100: not finite
    assert reproject_t(torch.tensor([[[100.0, 1.0]]]), Qinf)[1].tolist() == [[[False, True]]]


def test_well_conditioned_says_no():
    ops = ecm().ops
    assert well_conditioned(ops.q_matrix(700.0, 0.5, 31.37, 20.81), 40, 60)
    assert not well_conditioned(ops.q_matrix(700.0, 0.5, 31.0, 20.81), 40, 60)           # x = 31 sits on cx
    assert not well_conditioned(ops.q_matrix(700.0, 0.5, 31.37, 20.81, cx_right=30.0), 40, 60)   # Q33 < 0: W can cancel
    skew = ops.q_matrix(700.0, 0.5, 31.37, 20.81)
    skew[3, 0] = 1e-3
    assert not well_conditioned(skew, 40, 60)


# ---- the second ABI table: the census is tests/test_abi_types.py's, run over every table; what is this op's own stays here -----------
def geometry_header():
    return header_prototypes("ecm_geometry.h")


def test_geometry_prototypes_match_their_header_type_by_type():
    parsed = geometry_header()
    _I, _LL, _F, _P = C.c_int, C.c_longlong, C.c_float, C.c_void_p
    assert parsed["ecmg_point_cloud_scratch_bytes"] == (_LL, [_I, _I, _I]) and parsed["ecmg_point_cloud_tile"] == (_I, [])
    assert parsed["ecmg_reproject_fwd"] == (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _F, _F, _P])


def test_null_pointers_are_rejected_without_touching_the_gpu(lib_mod):
    lib, parsed = lib_mod.load(), geometry_header()
    for name in ("ecmg_reproject_fwd", "ecmg_point_cloud_fwd"):
        res, params = parsed[name]                                                        # laid out by the header, not by hand
        assert res is C.c_int
        args = [None if t is C.c_void_p else C.c_longlong(1 << 20) if t is C.c_longlong else 1.0 if t is C.c_float else 1 for t in params]
        assert getattr(lib, name)(*args) == -1, name
    p, q, o = C.c_void_p(64), C.c_void_p(4096), C.c_void_p(8192)                          # never dereferenced: every call returns first
    dense = lambda *tail: lib.ecmg_reproject_fwd(p, None, q, 0, o, None, *tail, None)     # noqa: E731
    assert dense(1, 1, 0, 0.0, 1.0) == -1 and dense(0, 1, 1, 0.0, 1.0) == -1 and dense(1, -1, 1, 0.0, 1.0) == -1
    assert dense(1, 1, 1, NAN, 1.0) == -1 and dense(1, 1, 1, INF, INF) == -1 and dense(1, 1, 1, 0.0, NAN) == -1
    assert dense(1, 1, 1, 2.0, 1.0) == -1
    assert lib.ecmg_reproject_fwd(p, None, q, 0, p, None, 1, 1, 1, 0.0, 1.0, None) == -1   # in place
    assert dense(1 << 15, 1 << 8, 1 << 8, 0.0, INF) == -2                                 # B * H * W = 2^31
    assert dense(1, 1 << 15, 1 << 16, 0.0, INF) == -2
    cloud = lambda C_, attrs, nb, *tail: lib.ecmg_point_cloud_fwd(p, None, q, 0, attrs, C_, o, C.c_void_p(12288), None, None,   # noqa: E731
                                                                  C.c_void_p(16384), C.c_longlong(nb), *tail, None)
    assert cloud(5, q, 1 << 20, 1, 4, 4, 0.0, 1.0) == -1 and cloud(-1, None, 1 << 20, 1, 4, 4, 0.0, 1.0) == -1
    assert cloud(2, None, 1 << 20, 1, 4, 4, 0.0, 1.0) == -1                               # C > 0 without planes
    assert cloud(0, None, 1 << 20, 1, 4, 0, 0.0, 1.0) == -1
    assert cloud(0, None, 0, 1, 4, 4, 0.0, 1.0) == -3 and cloud(0, None, 15, 2, 64, 64, 0.0, 1.0) == -3
    assert cloud(0, None, 1 << 20, 1 << 15, 1 << 8, 1 << 8, 0.0, INF) == -2


def test_tile_and_scratch_queries_need_no_gpu(lib_mod):
    k = kernel_constants()
    tile = lib_mod.query("ecmg_point_cloud_tile")
    assert tile == k["TILE"] == k["THREADS"] * k["ITEMS"] == ecm().ops.point_cloud_tile()
    assert k["WAVE"] == 64 and k["NWAVE"] * k["WAVE"] == k["THREADS"] and tile % 64 == 0
    nb = lambda B, H, W: lib_mod.query("ecmg_point_cloud_scratch_bytes", B, H, W)         # noqa: E731
    assert nb(1, 1, 1) == 16 and nb(1, 1, tile) == 16 and nb(1, 1, 4 * tile + 1) == 32    # one int per tile, in 16-byte steps
    assert nb(3, 33, 130) == 16 * -(-(3 * -(-33 * 130 // tile)) * 4 // 16)
    assert nb(4, 576, 960) == 4 * (576 * 960 // tile) * 4
    assert nb(0, 4, 4) == 0 and nb(1, 0, 4) == 0 and nb(1, 4, -1) == 0
    assert nb(1 << 15, 1 << 8, 1 << 8) == 0 and nb(1, 46341, 46341) == 0                  # B * H * W > INT_MAX
    assert nb(1, 32768, 65535) > 0                                                        # 2^31 - 2^15 pixels: taken
    assert nb(k["MAX_TILES"] + 1, 1, 1) == 0 and nb(k["MAX_TILES"], 1, 1) == 4 * (k["MAX_TILES"] + 1)


# ---- the refusals that come before any device work: all of this runs on CPU tensors -----------------------------------------------------
class OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the shape and dtype contract is checked before anything is launched."""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


def test_q_matrix_refusals():
    q_matrix = ecm().ops.q_matrix
    sig = inspect.signature(q_matrix)
    assert list(sig.parameters) == ["focal", "baseline", "cx", "cy", "cx_right", "x0", "y0"]
    assert [sig.parameters[n].default for n in ("cx_right", "x0", "y0")] == [None, 0, 0]
    for bad in ((0.0, 1.0, 1.0, 1.0), (700.0, 0.0, 1.0, 1.0), (700.0, -0.5, 1.0, 1.0), (NAN, 1.0, 1.0, 1.0), (700.0, 1.0, INF, 1.0),
                (700.0, 1.0, 1.0, "1"), (True, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="q_matrix"):
            q_matrix(*bad)
    with pytest.raises(ValueError, match="cx_right"):
        q_matrix(700.0, 1.0, 1.0, 1.0, cx_right=NAN)


@pytest.mark.parametrize("op", ["disparity_reproject", "point_cloud"])
def test_op_refusals(op):
    ops = ecm().ops
    fn = getattr(ops, op)
    Q = ops.q_matrix(700.0, 0.5, 31.37, 20.81)
    d = fake(2, 4, 8)
    for bad in (torch.zeros(4, 3), torch.zeros(3, 4, 4).flatten(), torch.zeros(2, 2, 4, 4), torch.zeros(0, 4, 4),
                torch.zeros(4, 4, dtype=torch.int64), Q.tolist(), None):
        with pytest.raises(ValueError, match="Q "):
            fn(d, bad)
    with pytest.raises(ValueError, match="one per image"):
        fn(d, torch.stack([Q] * 3))                                                       # [3,4,4] against B = 2
    for entry in (NAN, INF, -INF):
        bad = Q.clone()
        bad[1, 2] = entry
        with pytest.raises(ValueError, match="non-finite"):
            fn(d, bad)
        with pytest.raises(ValueError, match="non-finite"):
            fn(d, torch.stack([Q, bad]).float())
    for bad in (NAN, INF, -INF, None, "0", True, 1e39):
        with pytest.raises(ValueError, match="min_disp"):
            fn(d, Q, min_disp=bad)
    for lo, hi in ((2.0, 1.0), (0.0, -1.0), (0.0, NAN), (0.0, "9"), (1.0, -INF)):
        with pytest.raises(ValueError, match="max_disp"):
            fn(d, Q, min_disp=lo, max_disp=hi)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fn(torch.zeros(2, 4, 8), Q)
    for bad in (fake(4, 8), fake(2, 2, 4, 8), fake(8), fake(2, 0, 8)):
        with pytest.raises(RuntimeError, match=op):
            fn(bad, Q)
    with pytest.raises(RuntimeError, match="fp32"):
        fn(fake(2, 4, 8, dtype=torch.float64), Q)
    for bad in (fake(2, 4, 7, dtype=torch.bool), fake(1, 4, 8, dtype=torch.uint8), fake(2, 2, 4, 8, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match="valid"):
            fn(d, Q, valid=bad)
    with pytest.raises(RuntimeError, match="valid"):
        fn(d, Q, valid=fake(2, 4, 8))                                                     # a float plane is not a mask
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fn(d, Q, valid=torch.ones(2, 4, 8, dtype=torch.bool))


def test_point_cloud_attribute_refusals():
    ops = ecm().ops
    Q, d = ops.q_matrix(700.0, 0.5, 31.37, 20.81), fake(2, 4, 8)
    sig = inspect.signature(ops.point_cloud)
    assert list(sig.parameters) == ["disp", "Q", "attributes", "valid", "min_disp", "max_disp", "with_dense"]
    assert list(inspect.signature(ops.disparity_reproject).parameters) == ["disp", "Q", "valid", "min_disp", "max_disp", "with_mask"]
    with pytest.raises(ValueError, match="attribute planes"):
        ops.point_cloud(d, Q, fake(2, 5, 4, 8))                                           # C > 4
    for bad in (fake(2, 3, 4, 7), fake(1, 3, 4, 8), fake(2, 3, 5, 8), fake(3, 4, 8), fake(2, 4, 8)):
        with pytest.raises(RuntimeError, match="attributes"):
            ops.point_cloud(d, Q, bad)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.point_cloud(d, Q, fake(2, 3, 4, 8, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.point_cloud(d, Q, torch.zeros(2, 3, 4, 8))


def test_model_point_cloud_refuses_before_any_device_work():
    import ecm_amd
    from ecm_amd import models
    assert models.PointCloud._fields == ("points", "offsets", "xyz", "mask", "stage")
    assert tuple(models.POINT_CLOUD_SOURCES) == ("forward", "self_check", "cross_check", "refine", "despeckle", "smooth")
    sig = inspect.signature(models._ECMNet.point_cloud)
    assert list(sig.parameters) == ["self", "left", "right", "Q", "colors", "source", "min_disp", "max_disp", "stage_args"]
    assert [sig.parameters[n].default for n in ("colors", "source", "min_disp", "max_disp")] == [None, "smooth", 0.0, None]
    assert all(hasattr(cls, "point_cloud") for cls in models._MODELS.values())
    Q = ecm_amd.ops.q_matrix(700.0, 0.5, 31.37, 20.81)
    x = torch.zeros(1, 3, 64, 128)                                                        # CPU tensors, a model never moved
    for arch in ("cmfsm", "cmf"):
        net = ecm_amd.get_model(arch)
        for bad in ("wls", "", None, 2, "Smooth", "predict"):
            with pytest.raises(ValueError, match="source"):
                net.point_cloud(x, x, Q, source=bad)
        with pytest.raises(ValueError, match="Q "):
            net.point_cloud(x, x, torch.zeros(3, 3))
        with pytest.raises(ValueError, match="min_disp"):
            net.point_cloud(x, x, Q, min_disp=NAN)
        with pytest.raises(ValueError, match="max_disp"):
            net.point_cloud(x, x, Q, source="forward", min_disp=1.0, max_disp=0.5)
        with pytest.raises(ValueError, match="attribute planes"):
            net.point_cloud(x, x, Q, colors=torch.zeros(1, 5, 64, 128))
        with pytest.raises(ValueError, match="lam"):                                      # the stage's own refusals still come first
            net.point_cloud(x, x, Q, source="smooth", lam=0.0)
        with pytest.raises(RuntimeError):                                                 # and a forward on CPU tensors raises
            net.point_cloud(x, x, Q, source="forward")
