"""Stereo rectification, the part that needs no GPU: `rectify_map_t` and `remap_t` below, torch restatements
of the definitions in include/ecm_rectify.h -- the references of tests/test_hip_rectify.py -- checked against closed forms and at
the edges of the mask; ops.stereo_rectify's properties and its closed loop through the camera model; the signatures of the third
ABI table's entries (ENTRIES below; the census of _lib.RECTIFY_PROTOTYPES against include/ecm_rectify.h is
tests/test_abi_types.py's); and the refusals that come before any device work.

The map.  For output pixel (u, v): [X Y W] = iR [u v 1] with iR = (P[:, :3] R)^-1, x = X/W, y = Y/W, the rational radial and
tangential distortion of (x, y), then mx = fx xd + cx, my = fy yd + cy: every operation one fp64 operation in the order the
header gives, the two results rounded once to fp32.
The remap.  x0 = floor(mx), ax = mx - x0 (fp32, exact), likewise in y; the four taps as fp32, `border` outside the source;
top = t00 + ax (t01 - t00), bot = t10 + ax (t11 - t10), s = top + ay (bot - top); out = (s / 255 - mean) / std; mask = finite and
all four taps inside."""
import ctypes as C
import inspect
import math

import pytest
import torch

from frame_fixtures import MEAN, STD, loader_statements, raw_views as frames
from test_abi_types import header_prototypes, lib_mod  # noqa: F401  (lib_mod: a fixture)

ENTRIES = ("ecmr_rectify_map_fwd", "ecmr_rectify_map_params", "ecmr_remap_pair_fwd", "ecmr_tile_width")
NAN, INF = float("nan"), float("inf")
F64 = torch.float64


def ecm():
    import ecm_amd
    return ecm_amd


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def coefficients(D):
    """k1 k2 p1 p2 k3 k4 k5 k6 of a 4-, 5- or 8-vector in OpenCV's order."""
    return D.tolist() + [0.0] * (8 - len(D))


def rectify_map_t(K, D, R, P, new_size):
    """(map [2,Ho,Wo] fp32, map64 [2,Ho,Wo] before the rounding): the header's operations, one torch fp64 operation each."""
    Ho, Wo = new_size
    iR = torch.linalg.inv(P[:, :3] @ R).reshape(9).tolist()
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(D)
    u = torch.arange(Wo, dtype=F64).view(1, Wo).expand(Ho, Wo)
    v = torch.arange(Ho, dtype=F64).view(Ho, 1).expand(Ho, Wo)
    X = (iR[0] * u + iR[1] * v) + iR[2]
    Y = (iR[3] * u + iR[4] * v) + iR[5]
    W = (iR[6] * u + iR[7] * v) + iR[8]
    x, y = X / W, Y / W
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    r4 = r2 * r2
    r6 = r4 * r2
    xy2 = 2.0 * (x * y)
    radial = (((1.0 + k1 * r2) + k2 * r4) + k3 * r6) / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6)
    xd = x * radial + (p1 * xy2 + p2 * (r2 + 2.0 * x2))
    yd = y * radial + (p1 * (r2 + 2.0 * y2) + p2 * xy2)
    map64 = torch.stack([fx * xd + cx, fy * yd + cy])
    return map64.to(torch.float32), map64


def remap_t(raw, mp, mean=MEAN, std=STD, border=0.0, dtype=F64):
    """(out [B,3,Ho,Wo], image [B,3,Ho,Wo], mask [B,Ho,Wo] bool) of one view, the arithmetic in `dtype`: float64 is the reference,
    float32 the same formula at the kernel's precision.  raw: uint8 [B,H,W,3] or float32 [B,3,H,W]; mp: fp32 [2,Ho,Wo] or
    [B,2,Ho,Wo]; mean and std enter as their fp32 values."""
    assert mp.dtype == torch.float32
    src = (raw.permute(0, 3, 1, 2) if raw.dtype == torch.uint8 else raw).to(dtype)
    B, _, H, W = src.shape
    m = mp if mp.dim() == 4 else mp.unsqueeze(0).expand(B, -1, -1, -1)
    Ho, Wo = m.shape[-2:]
    mx, my = m[:, 0], m[:, 1]
    fin = torch.isfinite(mx) & torch.isfinite(my)
    mx, my = torch.where(fin, mx, torch.zeros_like(mx)), torch.where(fin, my, torch.zeros_like(my))
    fx0, fy0 = torch.floor(mx), torch.floor(my)
    ax, ay = (mx - fx0).to(dtype).unsqueeze(1), (my - fy0).to(dtype).unsqueeze(1)         # exact in fp32
    x0, y0 = fx0.clamp(-2, 2 ** 24).long(), fy0.clamp(-2, 2 ** 24).long()
    edge = torch.tensor(border, dtype=torch.float32).to(dtype)
    flat = src.reshape(B, 3, H * W)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, Ho * Wo).expand(B, 3, Ho * Wo)
        return torch.where(ok.unsqueeze(1), flat.gather(2, idx).view(B, 3, Ho, Wo), edge), ok

    (t00, k00), (t01, k01), (t10, k10), (t11, k11) = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = t00 + ax * (t01 - t00)
    bot = t10 + ax * (t11 - t10)
    s = top + ay * (bot - top)
    s = torch.where(fin.unsqueeze(1), s, edge)
    image = s / 255.0
    mean_t = torch.tensor(mean, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    std_t = torch.tensor(std, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return (image - mean_t) / std_t, image, fin & k00 & k01 & k10 & k11


def integer_map(Ho, Wo, dx=0, dy=0):
    x = torch.arange(Wo, dtype=torch.float32).view(1, Wo).expand(Ho, Wo) + dx
    y = torch.arange(Ho, dtype=torch.float32).view(Ho, 1).expand(Ho, Wo) + dy
    return torch.stack([x, y]).contiguous()


# ---- the rig of the tests -----------------------------------------------------------------------------------------------------------
def rotation(ax, ay, az):
    """Rz Ry Rx of three angles in radians, fp64."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=F64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=F64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=F64)
    return Rz @ Ry @ Rx


def rig(n_coefficients=5, size=(48, 64), rotated=True):
    """About 3 degrees about each axis and T = (-0.54, 0.01, -0.02); every distortion coefficient non-zero."""
    H, W = size
    K1 = torch.tensor([[1.31 * W, 0, 0.49 * W + 0.3], [0, 1.29 * W, 0.52 * H - 0.2], [0, 0, 1]], dtype=F64)
    K2 = torch.tensor([[1.27 * W, 0, 0.51 * W - 0.4], [0, 1.30 * W, 0.47 * H + 0.1], [0, 0, 1]], dtype=F64)
    D1 = torch.tensor([-0.21, 0.083, 0.0011, -0.0007, -0.013, 0.031, -0.012, 0.0021], dtype=F64)[:n_coefficients]
    D2 = torch.tensor([-0.19, 0.071, -0.0009, 0.0013, 0.009, 0.027, 0.011, -0.0017], dtype=F64)[:n_coefficients]
    d = math.radians(3.0)
    R = rotation(d, -1.1 * d, 0.9 * d) if rotated else torch.eye(3, dtype=F64)
    T = torch.tensor([-0.54, 0.01, -0.02], dtype=F64) if rotated else torch.tensor([-0.54, 0.0, 0.0], dtype=F64)
    return K1, D1, K2, D2, R, T, size


def project(X, K, D):
    """Pixels [N,2] of camera-frame points X [N,3] through the pinhole + distortion model, fp64."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(D)
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return torch.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1)


# ---- ops.stereo_rectify ---------------------------------------------------------------------------------------------------------------
def test_rectification_properties():
    ops = ecm().ops
    K1, D1, K2, D2, R, T, size = rig()
    assert float((R @ R.T - torch.eye(3, dtype=F64)).abs().max()) < 1e-15
    r = ops.stereo_rectify(K1, D1, K2, D2, R, T, size)
    assert isinstance(r, ops.Rectification) and r._fields == ("R1", "R2", "P1", "P2", "Q", "size", "new_size")
    eye = torch.eye(3, dtype=F64)
    for Rn in (r.R1, r.R2):
        assert Rn.dtype == F64 and float((Rn @ Rn.T - eye).abs().max()) <= 1e-14 and abs(float(torch.linalg.det(Rn)) - 1) <= 1e-14
    assert float((r.R2 @ R @ r.R1.T - eye).abs().max()) <= 1e-14
    norm = float(torch.linalg.vector_norm(T))
    assert float((r.R2 @ T - torch.tensor([-norm, 0, 0], dtype=F64)).abs().max()) <= 1e-14 * norm
    # the project's rule for the intrinsics
    f, cx, cy = min(float(K1[1, 1]), float(K2[1, 1])), float(K1[0, 2] + K2[0, 2]) / 2, float(K1[1, 2] + K2[1, 2]) / 2
    tx = float((r.R2 @ T)[0])
    want_P1 = torch.tensor([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]], dtype=F64)
    assert torch.equal(r.P1, want_P1) and torch.equal(r.P2[:, :3], want_P1[:, :3]) and r.P2[:, 3].tolist() == [f * tx, 0.0, 0.0]
    assert torch.equal(r.Q, ops.q_matrix(f, abs(tx), cx, cy)) and r.Q.dtype == F64          # bit for bit
    assert r.size == size and r.new_size == size


def test_new_size_focal_and_center():
    ops = ecm().ops
    K1, D1, K2, D2, R, T, size = rig()
    r = ops.stereo_rectify(K1, D1, K2, D2, R, T, size, new_size=(24, 48))
    f = min(float(K1[1, 1]), float(K2[1, 1])) * (24 / 48)
    cx, cy = float(K1[0, 2] + K2[0, 2]) / 2 * (48 / 64), float(K1[1, 2] + K2[1, 2]) / 2 * (24 / 48)
    assert r.P1[0, 0] == f and r.P1[1, 1] == f and r.P1[0, 2] == cx and r.P1[1, 2] == cy and r.new_size == (24, 48)
    r = ops.stereo_rectify(K1, D1, K2, D2, R, T, size, focal=77.5, center=(30.25, 20.5))
    assert r.P1[0, 0] == 77.5 and r.P2[1, 1] == 77.5 and r.P2[0, 2] == 30.25 and r.P1[1, 2] == 20.5
    assert torch.equal(r.Q, ops.q_matrix(77.5, abs(float((r.R2 @ T)[0])), 30.25, 20.5))


def test_an_aligned_rig_is_left_alone():
    ops = ecm().ops
    K1, D1, K2, D2, R, T, size = rig(rotated=False)
    r = ops.stereo_rectify(K1, D1, K2, D2, R, T, size)
    eye = torch.eye(3, dtype=F64)
    assert torch.equal(r.R1, eye) and torch.equal(r.R2, eye)                               # exactly
    assert float(r.P2[0, 3]) == float(r.P1[0, 0]) * -0.54


def test_rodrigues_round_trip():
    ops = ecm().ops
    for om in ([0.0, 0.0, 0.0], [1e-11, -2e-11, 0.5e-11], [0.3, -0.2, 0.1], [2.0, 1.5, -1.0], [math.pi, 0.0, 0.0],
               [0.0, -math.pi * 0.6, math.pi * 0.8]):
        om = torch.tensor(om, dtype=F64)
        Rm = ops._rotation_matrix(om)
        assert float((Rm @ Rm.T - torch.eye(3, dtype=F64)).abs().max()) < 1e-15
        back = ops._rotation_matrix(ops._rotation_vector(Rm))
        assert float((back - Rm).abs().max()) < 1e-14, om


@pytest.mark.parametrize("n", [4, 5, 8])
def test_closed_loop_through_the_camera_model(n):
    """Q [u v d 1] is a point of the rectified left frame; rotated back and projected through (K1, D1) it is the left map at
    (u, v), moved through (R, T) and projected through (K2, D2) it is the right map at (u - d, v): stereo_rectify, the map
    definition and Q hold each other, with nothing but the pinhole-plus-distortion model between them.  fp64, 1e-9 px."""
    ops = ecm().ops
    K1, D1, K2, D2, R, T, size = rig(n)
    r = ops.stereo_rectify(K1, D1, K2, D2, R, T, size)
    H, W = size
    _, left64 = rectify_map_t(K1, D1, r.R1, r.P1, size)
    _, right64 = rectify_map_t(K2, D2, r.R2, r.P2, size)
    us, vs, ds = torch.meshgrid(torch.arange(0, W, 3), torch.arange(0, H, 5), torch.tensor([1, 4, 17]), indexing="ij")
    keep = us - ds >= 0
    u, v, d = us[keep], vs[keep], ds[keep]
    assert len(u) > 300
    h = r.Q @ torch.stack([u, v, d, torch.ones_like(u)]).to(F64)                            # [4,N]
    Xr = (h[:3] / h[3]).T                                                                   # rectified left frame
    X1 = Xr @ r.R1                                                                          # = (R1^T Xr^T)^T
    got_left = project(X1, K1, D1)
    want_left = left64[:, v, u].T
    X2 = X1 @ R.T + T
    got_right = project(X2, K2, D2)
    want_right = right64[:, v, u - d].T
    worst = max(float((got_left - want_left).abs().max()), float((got_right - want_right).abs().max()))
    print(f"RECTIFY closed loop, {n} coefficients, {len(u)} points: worst {worst:.3e} px")
    assert worst <= 1e-9


def test_map_parameters_are_the_restatements_numbers(lib_mod):
    ops = ecm().ops
    K1, D1, K2, D2, R, T, size = rig(5)
    r = ops.stereo_rectify(K1, D1, K2, D2, R, T, size)
    p = ops.rectify_map_params(K2, D2, r.R2, r.P2)
    assert p.dtype == F64 and p.shape == (21,) == (ecm()._lib.query("ecmr_rectify_map_params"),)
    assert torch.equal(p[:9], torch.linalg.inv(r.P2[:, :3] @ r.R2).reshape(9))              # the nine doubles of rectify_map_t
    assert p[9:13].tolist() == [float(K2[0, 0]), float(K2[1, 1]), float(K2[0, 2]), float(K2[1, 2])]
    assert p[13:].tolist() == coefficients(D2)
    assert ops.rectify_map_params(K2, D2[:4], r.R2, r.P2)[13:].tolist() == D2[:4].tolist() + [0.0] * 4
    # an undistorted camera under the identity maps every pixel onto itself
    K = K1.clone()
    ident, ident64 = rectify_map_t(K, torch.zeros(4, dtype=F64), torch.eye(3, dtype=F64), torch.cat([K, torch.zeros(3, 1, dtype=F64)], 1), (6, 9))
    assert float((ident64 - integer_map(6, 9).to(F64)).abs().max()) < 1e-12 and torch.equal(ident, ident64.to(torch.float32))


# ---- remap_t against closed forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_identity_map_is_the_normalised_input(kind):
    raw = frames(2, 5, 7, 3, kind)
    out, image, mask = remap_t(raw, integer_map(4, 6))                                     # the last row and column need outside taps
    want = loader_statements(frames(2, 5, 7, 3))[1]                                        # ops.frame_prep's planes
    assert float((out - want[:, :, :4, :6].to(F64)).abs().max()) < 1e-6
    assert torch.equal(remap_t(raw, integer_map(4, 6), dtype=torch.float32)[0], want[:, :, :4, :6])
    assert bool(mask.all()) and mask.shape == (2, 4, 6) and mask.dtype == torch.bool
    assert torch.equal(image, frames(2, 5, 7, 3).permute(0, 3, 1, 2)[:, :, :4, :6].to(F64) / 255.0)
    full32, _, full_mask = remap_t(raw, integer_map(5, 7), dtype=torch.float32)             # weight-0 taps outside: same values
    assert torch.equal(full32, want) and torch.equal(full_mask[0], (integer_map(5, 7)[0] < 6) & (integer_map(5, 7)[1] < 4))


def test_integer_shift_moves_the_image():
    raw = frames(1, 5, 9, 4)
    out, _, mask = remap_t(raw, integer_map(5, 9, dx=-2), border=37.0, dtype=torch.float32)
    want = loader_statements(raw)[1]
    edge = ((torch.tensor(37.0) / 255.0 - torch.tensor(MEAN)) / torch.tensor(STD)).view(1, 3, 1, 1)
    assert torch.equal(out[..., 2:], want[..., :-2]) and torch.equal(out[..., :2], edge.expand(1, 3, 5, 2))
    assert not bool(mask[..., :2].any()) and bool(mask[:, :4, 2:].all()) and not bool(mask[:, 4].any())


def test_half_pixel_shift_is_the_mean_of_neighbours():
    raw = frames(1, 4, 8, 5)
    v = raw.permute(0, 3, 1, 2).to(F64)
    _, image, mask = remap_t(raw, integer_map(3, 7, dx=0.5, dy=0.5))
    want = (v[..., :-1, :-1] + v[..., :-1, 1:] + v[..., 1:, :-1] + v[..., 1:, 1:]) / 4 / 255.0
    assert float((image - want).abs().max()) < 1e-15 and bool(mask.all())
    _, image, _ = remap_t(raw, integer_map(4, 7, dx=0.5))
    assert float((image - (v[..., :-1] + v[..., 1:]) / 2 / 255.0).abs().max()) < 1e-15


BOUNDARY_W = 6
#            coordinate, inside, what the sample is (as an expression of the row r[0..W-1] and the border e)
BOUNDARY = [(-1.0, False, lambda r, e: e),
            (-2.0 ** -10, False, lambda r, e: e + (1 - 2.0 ** -10) * (r[0] - e)),
            (0.0, True, lambda r, e: r[0]),
            (BOUNDARY_W - 2.0, True, lambda r, e: r[BOUNDARY_W - 2]),
            (BOUNDARY_W - 1.0, False, lambda r, e: r[BOUNDARY_W - 1]),                     # on the last column: not inside
            (BOUNDARY_W - 1 + 2.0 ** -10, False, lambda r, e: r[BOUNDARY_W - 1] + 2.0 ** -10 * (e - r[BOUNDARY_W - 1])),
            (float(BOUNDARY_W), False, lambda r, e: e),
            (NAN, False, lambda r, e: e), (INF, False, lambda r, e: e), (-INF, False, lambda r, e: e),
            (1e30, False, lambda r, e: e), (-1e30, False, lambda r, e: e)]


def boundary_maps():
    """(map along x at row 1, map along y at column 1) over a BOUNDARY_W x BOUNDARY_W source."""
    c = torch.tensor([b[0] for b in BOUNDARY], dtype=torch.float32).view(1, -1)
    one = torch.ones_like(c)
    return torch.stack([c, one]), torch.stack([one, c])


def test_boundary_coordinates_land_on_the_documented_side():
    raw = frames(1, BOUNDARY_W, BOUNDARY_W, 6)
    v = raw.permute(0, 3, 1, 2).to(F64)
    along_x, along_y = boundary_maps()
    e = 11.0
    for mp, line in ((along_x, v[0, :, 1, :]), (along_y, v[0, :, :, 1])):                  # line [3, W]
        _, image, mask = remap_t(raw, mp, border=e)
        assert mask[0, 0].tolist() == [b[1] for b in BOUNDARY]
        for k, (_, _, value) in enumerate(BOUNDARY):
            for ch in range(3):
                assert abs(float(image[0, ch, 0, k]) * 255.0 - float(value(line[ch].tolist(), e))) < 1e-12, (k, ch)


# ---- the third ABI table: the census is tests/test_abi_types.py's, run over every table; what is this op's own stays here -------------
def rectify_header():
    return header_prototypes("ecm_rectify.h")


def test_rectify_prototypes_match_their_header_type_by_type():
    parsed = rectify_header()
    _I, _F, _P = C.c_int, C.c_float, C.c_void_p
    assert parsed["ecmr_rectify_map_fwd"] == (_I, [_P, _P, _I, _I, _P]) and parsed["ecmr_tile_width"] == (_I, [])
    assert parsed["ecmr_remap_pair_fwd"] == (_I, [_P, _P, _I, _P, _P, _I] + [_P] * 5 + [_I] * 5 + [_P, _P, _F, _P])


def test_queries_need_no_gpu(lib_mod):
    assert lib_mod.query("ecmr_rectify_map_params") == 21
    assert lib_mod.query("ecmr_tile_width") == 64 == ecm().ops.rectify_tile_width()


def test_the_abi_refuses_without_touching_the_gpu(lib_mod):
    lib, parsed = lib_mod.load(), rectify_header()
    for name in ("ecmr_rectify_map_fwd", "ecmr_remap_pair_fwd"):
        res, params = parsed[name]                                                          # laid out by the header, not by hand
        assert res is C.c_int
        args = [None if t is C.c_void_p else 1.0 if t is C.c_float else 1 for t in params]
        assert getattr(lib, name)(*args) == -1, name
    P = lambda n: C.c_void_p(n << 30)                                                       # noqa: E731  never dereferenced: 1 GiB apart
    assert lib.ecmr_rectify_map_fwd(P(1), P(2), 0, 4, None) == -1 and lib.ecmr_rectify_map_fwd(P(1), P(2), 4, -1, None) == -1
    assert lib.ecmr_rectify_map_fwd(P(1), P(1), 4, 4, None) == -1                            # in place
    assert lib.ecmr_rectify_map_fwd(P(1), C.c_void_p((1 << 30) - 64), 4, 4, None) == -1      # the map runs into the parameters
    assert lib.ecmr_rectify_map_fwd(P(1), P(2), 1 << 16, 1 << 15, None) == -2                # Ho * Wo = 2^31
    assert lib.ecmr_rectify_map_fwd(P(1), P(2), 262141, 1, None) == -2
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    host = lambda a: C.cast(a, C.c_void_p)                                                  # noqa: E731

    def remap(ptrs=None, dims=(1, 5, 7, 3, 5), u8=1, per_image=0, mean=m3, std=s3, border=0.0):
        p = {"lr": P(1), "rr": P(2), "ml": P(3), "mr": P(4), "l": P(5), "r": P(6), "im": P(7), "kl": P(8), "kr": P(9)}
        p.update(ptrs or {})
        return lib.ecmr_remap_pair_fwd(p["lr"], p["rr"], u8, p["ml"], p["mr"], per_image, p["l"], p["r"], p["im"], p["kl"], p["kr"],
                                       *dims, host(mean) if mean is not None else None, host(std) if std is not None else None,
                                       border, None)

    for missing in ("lr", "rr", "ml", "mr", "l", "r"):
        assert remap({missing: None}) == -1, missing
    assert remap(mean=None) == -1 and remap(std=None) == -1
    for dims in ((0, 5, 7, 3, 5), (1, 0, 7, 3, 5), (1, 5, -1, 3, 5), (1, 5, 7, 0, 5), (1, 5, 7, 3, 0)):
        assert remap(dims=dims) == -1, dims
    for border in (NAN, INF, -INF):
        assert remap(border=border) == -1
    assert remap(std=(C.c_float * 3)(0.2, 0.0, 0.2)) == -1 and remap(mean=(C.c_float * 3)(0.2, NAN, 0.2)) == -1
    # in place or overlapping: an output on an input, on another output, and running into one
    for out in ("l", "r", "im", "kl", "kr"):
        for other in ("lr", "rr", "ml", "mr"):
            assert remap({out: P({"lr": 1, "rr": 2, "ml": 3, "mr": 4}[other])}) == -1, (out, other)
    assert remap({"r": P(5)}) == -1 and remap({"im": P(6)}) == -1 and remap({"kr": P(8)}) == -1 and remap({"kl": P(5)}) == -1
    assert remap({"l": C.c_void_p((2 << 30) - 16)}) == -1 and remap({"r": C.c_void_p((5 << 30) + 3 * 3 * 5 * 4 - 4)}) == -1
    # B * max(H W, Ho Wo) >= 2^31 and the other limits: ECM_EUNSUP before any launch
    assert remap(dims=(1 << 15, 1 << 8, 1 << 8, 3, 5)) == -2 and remap(dims=(2, 3, 5, 1 << 15, 1 << 15)) == -2
    assert remap(dims=(1, 1, (1 << 24) + 1, 3, 5)) == -2 and remap(dims=(1, (1 << 24) + 1, 1, 3, 5)) == -2
    assert remap(dims=(32768, 1, 1, 1, 1)) == -2 and remap(dims=(1, 1, 1, 1048561, 1)) == -2


# ---- the refusals of the ops: all of this runs on CPU tensors ---------------------------------------------------------------------------
class OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the shape and dtype contract is checked before anything is launched."""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


def test_stereo_rectify_refusals():
    ops = ecm().ops
    sig = inspect.signature(ops.stereo_rectify)
    assert list(sig.parameters) == ["K1", "D1", "K2", "D2", "R", "T", "size", "new_size", "focal", "center"]
    assert [sig.parameters[n].default for n in ("new_size", "focal", "center")] == [None, None, None]
    good = dict(zip(("K1", "D1", "K2", "D2", "R", "T", "size"), rig()))
    ops.stereo_rectify(**good)

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            ops.stereo_rectify(**{**good, **change})

    for name in ("K1", "K2", "R"):                                                          # shapes and dtypes
        refused(name, **{name: good[name].float()})
        refused(name, **{name: good[name][:2]})
        refused(name, **{name: good[name].tolist()})
    for name in ("D1", "D2", "T"):
        refused(name, **{name: good[name].float()})
        refused(name, **{name: good[name].view(1, -1)})
    refused("T ", T=torch.zeros(4, dtype=F64))
    for name in ("K1", "D1", "K2", "D2", "R", "T"):                                         # non-finite entries
        for entry in (NAN, INF):
            bad = good[name].clone()
            bad.view(-1)[1] = entry
            refused("non-finite", **{name: bad})
    for n in (0, 3, 6, 7, 9, 12, 14):                                                       # len(D)
        refused("coefficients", D1=torch.zeros(n, dtype=F64))
        refused("coefficients", D2=torch.zeros(n, dtype=F64))
    skewed = good["K1"].clone()
    skewed[0, 1] = 0.5
    refused("pinhole", K1=skewed)
    tilted = good["R"].clone()
    tilted[0, 1] += 1e-5
    refused("not a rotation", R=tilted)
    refused("not a rotation", R=torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=F64)))
    nearly = good["R"].clone()
    nearly[0, 1] += 1e-9                                                                    # within 1e-6: taken
    ops.stereo_rectify(**{**good, "R": nearly})
    refused("T is zero", T=torch.zeros(3, dtype=F64))
    refused("vertical", T=torch.tensor([-0.1, 0.5, 0.0], dtype=F64))
    refused("swap the views", T=torch.tensor([0.54, 0.01, -0.02], dtype=F64))
    for bad in ((48,), (48, 64, 3), (0, 64), (48, -1), (48.0, 64), "48x64", None, (True, 64)):
        refused("size", size=bad)
        if bad is not None:
            refused("new_size", new_size=bad)
    for bad in (0.0, -1.0, NAN, INF, "700", True):
        refused("focal", focal=bad)
    for bad in ((1.0,), (1.0, NAN), (INF, 2.0), "c", 5.0, (1.0, 2.0, 3.0)):
        refused("center", center=bad)


def test_rectify_map_refusals():
    ops = ecm().ops
    assert list(inspect.signature(ops.rectify_map).parameters) == ["K", "D", "R", "P", "new_size", "device"]
    K1, D1, _, _, R, T, size = rig()
    r = ops.stereo_rectify(K1, D1, K1, D1, R, T, size)
    good = dict(K=K1, D=D1, R=r.R1, P=r.P1, new_size=size, device="cuda")

    def refused(exc, match, **change):
        with pytest.raises(exc, match=match):
            ops.rectify_map(**{**good, **change})

    refused(ValueError, "K ", K=K1.float())
    refused(ValueError, "D ", D=D1.view(1, -1))
    refused(ValueError, "coefficients", D=torch.zeros(6, dtype=F64))
    refused(ValueError, "R ", R=r.R1[:2])
    refused(ValueError, "P ", P=r.P1[:, :3])
    refused(ValueError, "P ", P=r.P1.float())
    bad = r.P1.clone()
    bad[1, 1] = NAN
    refused(ValueError, "non-finite", P=bad)
    flat = r.P1.clone()
    flat[1] = flat[0]
    refused(ValueError, "singular", P=flat)
    refused(ValueError, "singular", P=torch.zeros(3, 4, dtype=F64))
    for bad in ((0, 4), (4,), (4.0, 4), None):
        refused(ValueError, "new_size", new_size=bad)
    refused(RuntimeError, "no CPU fallback", device="cpu")
    refused(RuntimeError, "no CPU fallback", device=torch.device("cpu"))


def test_remap_pair_refusals():
    ops = ecm().ops
    sig = inspect.signature(ops.remap_pair)
    assert list(sig.parameters) == ["left_raw", "right_raw", "map_left", "map_right", "mean", "std", "border", "want_image", "with_mask"]
    assert [sig.parameters[n].default for n in ("mean", "std", "border", "want_image", "with_mask")] == \
        [ops.FLYING3D_MEAN, ops.FLYING3D_STD, 0.0, False, False]
    raw, mp = fake(2, 5, 7, 3, dtype=torch.uint8), fake(2, 3, 5)
    cpu_raw, cpu_map = torch.zeros(2, 5, 7, 3, dtype=torch.uint8), torch.zeros(2, 3, 5)
    for args in ((cpu_raw, raw, mp, mp), (raw, cpu_raw, mp, mp), (raw, raw, cpu_map, mp), (raw, raw, mp, cpu_map)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.remap_pair(*args)
    for bad in (fake(2, 5, 7, 4, dtype=torch.uint8), fake(5, 7, 3, dtype=torch.uint8), fake(2, 3, 5, 7, dtype=torch.float64),
                fake(2, 4, 5, 7), fake(2, 5, 7, 3, dtype=torch.int32), fake(0, 5, 7, 3, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="left_raw"):
            ops.remap_pair(bad, bad, mp, mp)
    for bad in (fake(2, 5, 8, 3, dtype=torch.uint8), fake(1, 5, 7, 3, dtype=torch.uint8), fake(2, 3, 5, 7)):
        with pytest.raises(RuntimeError, match="right_raw"):
            ops.remap_pair(raw, bad, mp, mp)
    for bad in (fake(3, 3, 5), fake(3, 5), fake(3, 2, 3, 5), fake(2, 3, 5, dtype=torch.float64), fake(1, 1, 2, 3, 5), fake(2, 0, 5)):
        with pytest.raises(RuntimeError, match="map_left"):
            ops.remap_pair(raw, raw, bad, bad)
    for bad in (fake(2, 3, 6), fake(2, 2, 3, 5), fake(2, 3, 5, dtype=torch.float16)):
        with pytest.raises(RuntimeError, match="map_right"):
            ops.remap_pair(raw, raw, mp, bad)
    for bad in (NAN, INF, -INF, None, "0", True, 1e39):
        with pytest.raises(ValueError, match="border"):
            ops.remap_pair(raw, raw, mp, mp, border=bad)
    for bad in ((0.5, 0.5), (0.5, NAN, 0.5), 0.5, (0.5, "a", 0.5)):
        with pytest.raises(ValueError, match="mean"):
            ops.remap_pair(raw, raw, mp, mp, mean=bad)
    for bad in ((0.2, 0.0, 0.2), (0.2, INF, 0.2), (0.2, 0.2)):
        with pytest.raises(ValueError, match="std"):
            ops.remap_pair(raw, raw, mp, mp, std=bad)


def test_stereo_rig_refuses_before_any_device_work():
    import ecm_amd
    from ecm_amd import models
    sig = inspect.signature(models.StereoRig.__init__)
    assert list(sig.parameters) == ["self", "K1", "D1", "K2", "D2", "R", "T", "size", "new_size", "focal", "center"]
    assert list(inspect.signature(models.StereoRig.__call__).parameters) == ["self", "left_raw", "right_raw", "want_image", "with_mask"]
    sig = inspect.signature(models.StereoRig.point_cloud)
    assert list(sig.parameters) == ["self", "model", "left_raw", "right_raw", "source", "colors", "stage_args"]
    assert [sig.parameters[n].default for n in ("source", "colors")] == ["smooth", "image"]
    assert not issubclass(models.StereoRig, torch.nn.Module)
    assert not any(hasattr(models._ECMNet, n) for n in ("rectify", "remap_pair", "rig", "stereo_rig"))   # no model method is added
    good = rig()
    r = models.StereoRig(*good, new_size=(24, 32))
    want = ecm_amd.ops.stereo_rectify(*good, new_size=(24, 32))
    assert all(torch.equal(a, b) for a, b in zip(r.rectification[:5], want[:5])) and r.rectification[5:] == want[5:]
    assert r.Q is r.rectification.Q
    with pytest.raises(ValueError, match="swap the views"):
        models.StereoRig(*good[:5], -good[5], good[6])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(torch.zeros(1, 48, 64, 3, dtype=torch.uint8), torch.zeros(1, 48, 64, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.maps("cpu")
    for bad in (fake(1, 48, 65, 3, dtype=torch.uint8), fake(1, 3, 47, 64), fake(48, 64, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="calibrated"):
            r(bad, bad)
    with pytest.raises(ValueError, match="colors"):
        r.point_cloud(ecm_amd.get_model("cmfsm"), fake(1, 48, 64, 3, dtype=torch.uint8), fake(1, 48, 64, 3, dtype=torch.uint8), colors="rgb")
