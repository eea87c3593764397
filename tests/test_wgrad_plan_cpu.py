"""The launch plans of the weight gradients (csrc/conv3d_wgrad.hip `plan<Cfg>`, csrc/conv3d_c1.hip and csrc/conv2d_c1.hip
`c1_wgrad_plan`), restated here in a few lines of Python and held against the five `*_scratch_bytes` queries of the library on a
grid that crosses every branch.  No GPU: the queries are host arithmetic.  The byte counts are part of the ABI's behaviour
(callers cache by them), so this restatement is the record of what they are; tests/test_hip_guard_bands.py imports it to
recompute the worker count P and the tile count of its cap-binding cases.

One departure from a plain product of {1, 32, 33, 64, 320}^2 channels: its largest pair has 10 x 10 = 100 channel tiles, which is
below 256, so the `workers < 1` clamp would never be taken; 544 (17 x 17 = 289 > 256) and 736 (23 x 23 = 529 > 512) are added
for it, one per occupancy."""
import os

import pytest

CT, TWV = 32, 16                                             # channel tile, tile width (csrc/conv3d_wgrad.hip)
MAX_KG_2D = 4                                                # partials per worker the general 2-D query promises
TILE_3D = {1: (2, 8), 2: (1, 4)}                             # stride -> (TD, TH), occupancy 1, one partial per worker
TILE_WINO = {3: (2, 8, 1), 1: (1, 16, 2)}                    # kd -> (TD, TH, occupancy)
TH_2D = {(3, 3, 1): 16, (3, 3, 2): 8, (3, 5, 1): 16, (1, 1, 1): 16, (1, 1, 2): 8}       # (kh, kw, stride) -> TH, occupancy 2
KG_2D = {9: 2, 15: 1, 1: 4}                                  # taps -> partials per worker the kernels write
C1_3D_TILE, C1_3D_CAP = (2, 8, 32), 512
C1_2D_TX, C1_2D_TY, C1_2D_SUB = 64, 32, 4


def cdiv(a, b):
    return -(-a // b)


def out(n, stride):
    return (n - 1) // stride + 1


def workers(ntiles, Ci, Co, occ):
    ytiles = cdiv(Ci, CT) * cdiv(Co, CT)
    return max(1, min(ntiles, 256 * occ // ytiles))


def ntiles(B, Do, Ho, Wo, TD, TH):
    return B * cdiv(Do, TD) * cdiv(Ho, TH) * cdiv(Wo, TWV)


def plan_3d(B, Ci, Co, D, H, W, stride):
    """-> (ntiles, P, bytes) of ecm_conv3d_k3_wgrad"""
    nt = ntiles(B, out(D, stride), out(H, stride), out(W, stride), *TILE_3D[stride])
    P = workers(nt, Ci, Co, 1)
    return nt, P, P * Co * Ci * 27 * 4


def plan_2d(B, Ci, Co, Ho, Wo, kh, kw, stride):
    """-> (ntiles, P, bytes) of ecm_conv2d_wgrad_ex; outside the table: the tile of the stride, the caller's taps"""
    nt = ntiles(B, 1, Ho, Wo, 1, TH_2D.get((kh, kw, stride), 16 if stride == 1 else 8))
    P = workers(nt, Ci, Co, 2)
    return nt, P, P * MAX_KG_2D * Co * Ci * kh * kw * 4


def plan_wino(B, Ci, Co, D, H, W, kd):
    """-> (ntiles, P, bytes) of ecm_conv_wino_wgrad: P partials and their sum, in the 16-frequency domain"""
    TD, TH, occ = TILE_WINO[kd]
    nt = ntiles(B, D, H, W, TD, TH)
    P = workers(nt, Ci, Co, occ)
    return nt, P, (P + 1) * 16 * kd * Co * Ci * 4


def plan_c1_3d(B, Ci, D, H, W):
    nt = B * cdiv(D, C1_3D_TILE[0]) * cdiv(H, C1_3D_TILE[1]) * cdiv(W, C1_3D_TILE[2])
    P = min(nt, C1_3D_CAP)
    return nt, P, P * Ci * 27 * 4


def plan_c1_2d(B, Ci, H, W):
    if B * cdiv(H, C1_2D_TY) * cdiv(W, C1_2D_TX) > 0x7fffffff or Ci > 4096:
        return 0, 0, 0
    P = B * cdiv(H, C1_2D_TY * C1_2D_SUB) * cdiv(W, C1_2D_TX)
    return P, P, P * (Ci * 9 + 1) * 4


CHANNELS = (1, 32, 33, 64, 320, 544, 736)
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)
RAGGED = ((1, 3, 9, 17), (2, 5, 17, 33), (1, 6, 32, 96), (3, 1, 1, 1), (4, 48, 144, 240), (1, 2, 4, 130))     # (B, D, H, W)
ROWS_2D = tuple(TH_2D) + ((5, 5, 1), (7, 7, 2), (3, 3, 3), (2, 3, 0))      # the last four: no kernel, the query still answers


def grid():
    """Every (query, arguments, expected bytes, (ntiles, cap) or None) of the comparison."""
    for Ci in CHANNELS:
        for Co in CHANNELS:
            yt = cdiv(Ci, CT) * cdiv(Co, CT)
            for stride in (1, 2):
                TD, TH = TILE_3D[stride]
                shapes = [(n, TD * stride, TH * stride, TWV * stride) for n in COUNTS] + list(RAGGED)
                for B, D, H, W in shapes:
                    nt, P, nb = plan_3d(B, Ci, Co, D, H, W, stride)
                    yield "ecm_conv3d_wgrad_scratch_bytes", (B, Ci, Co, D, H, W, stride), nb, (nt, 256 // yt)
            for kd in (3, 1):
                TD, TH, occ = TILE_WINO[kd]
                for B, D, H, W in [(n, TD, TH, TWV) for n in COUNTS] + list(RAGGED):
                    nt, P, nb = plan_wino(B, Ci, Co, D, H, W, kd)
                    yield "ecm_conv_wino_wgrad_scratch_bytes", (B, Ci, Co, D, H, W, kd), nb, (nt, 256 * occ // yt)
            for kh, kw, stride in ROWS_2D:
                th = TH_2D.get((kh, kw, stride), 16 if stride == 1 else 8)
                for B, _, Ho, Wo in [(n, 1, th, TWV) for n in COUNTS] + list(RAGGED):
                    nt, P, nb = plan_2d(B, Ci, Co, Ho, Wo, kh, kw, stride)
                    yield "ecm_conv2d_wgrad_ex_scratch_bytes", (B, Ci, Co, Ho, Wo, kh, kw, stride), nb, (nt, 512 // yt)
    for Ci in (1, 3, 32, 33, 4096):
        for B, D, H, W in [(n, 2, 8, 32) for n in COUNTS] + list(RAGGED):
            nt, P, nb = plan_c1_3d(B, Ci, D, H, W)
            yield "ecm_conv3d_c1_wgrad_scratch_bytes", (B, Ci, D, H, W), nb, (nt, C1_3D_CAP)
        for B, _, H, W in [(n, 1, 128, 64) for n in COUNTS] + list(RAGGED) + [(1, 1, 129, 65), (2, 1, 576, 960)]:
            yield "ecm_conv2d_c1_wgrad_scratch_bytes", (B, Ci, H, W), plan_c1_2d(B, Ci, H, W)[2], None
    yield "ecm_conv2d_c1_wgrad_scratch_bytes", (1, 4097, 8, 8), 0, None                      # Ci beyond the kernel's contract
    yield "ecm_conv2d_c1_wgrad_scratch_bytes", (1 << 20, 1, 1 << 16, 1 << 12), 0, None        # more than 2^31 tiles
    # every invalid argument answers 0
    good = {"ecm_conv3d_wgrad_scratch_bytes": (2, 32, 32, 4, 8, 16, 1), "ecm_conv_wino_wgrad_scratch_bytes": (2, 32, 32, 4, 8, 16, 3),
            "ecm_conv2d_wgrad_ex_scratch_bytes": (2, 32, 32, 8, 16, 3, 3, 1), "ecm_conv3d_c1_wgrad_scratch_bytes": (2, 32, 4, 8, 16),
            "ecm_conv2d_c1_wgrad_scratch_bytes": (2, 32, 8, 16)}
    sizes = {"ecm_conv3d_wgrad_scratch_bytes": 6, "ecm_conv_wino_wgrad_scratch_bytes": 6, "ecm_conv2d_wgrad_ex_scratch_bytes": 7,
             "ecm_conv3d_c1_wgrad_scratch_bytes": 5, "ecm_conv2d_c1_wgrad_scratch_bytes": 4}      # leading arguments that must be > 0
    for name, args in good.items():
        for i in range(sizes[name]):
            for bad in (0, -1):
                yield name, args[:i] + (bad,) + args[i + 1:], 0, None
    for stride in (0, 3, -1):
        yield "ecm_conv3d_wgrad_scratch_bytes", good["ecm_conv3d_wgrad_scratch_bytes"][:6] + (stride,), 0, None
    for kd in (0, 2, 4):
        yield "ecm_conv_wino_wgrad_scratch_bytes", good["ecm_conv_wino_wgrad_scratch_bytes"][:6] + (kd,), 0, None


@pytest.fixture(scope="module")
def lib_mod():
    import ecm_amd
    if not os.path.exists(ecm_amd._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm_amd._lib


def test_the_restatement_is_the_documented_one():
    """Spot values worked by hand, so that the restatement cannot drift together with the library."""
    assert plan_3d(1, 64, 64, 6, 32, 96, 1) == (72, 64, 64 * 64 * 64 * 27 * 4)            # 3 x 4 x 6 tiles, 256 // 4 workers
    assert plan_3d(4, 32, 32, 48, 144, 240, 1)[:2] == (4 * 24 * 18 * 15, 256)
    assert plan_3d(1, 544, 544, 4, 8, 16, 2)[:2] == (2 * 1 * 1, 1)                          # 289 channel tiles: clamped to 1
    assert plan_2d(2, 32, 32, 8, 16, 1, 1, 2) == (2, 2, 2 * 4 * 32 * 32 * 4)
    assert plan_wino(1, 32, 32, 1, 16, 16, 1) == (1, 1, 2 * 16 * 32 * 32 * 4)
    assert plan_c1_3d(4, 32, 48, 144, 240) == (4 * 24 * 18 * 8, 512, 512 * 32 * 27 * 4)
    assert plan_c1_2d(2, 32, 576, 960)[2] == 2 * 5 * 15 * 289 * 4
    assert all(KG_2D[kh * kw] <= MAX_KG_2D for kh, kw, _ in TH_2D)


def test_the_grid_crosses_every_branch():
    seen = {}
    for name, args, want, cap in grid():
        s = seen.setdefault(name, set())
        s.add("zero" if want == 0 else "answer")
        if cap is not None:
            nt, c = cap
            s.add("clamp" if c < 1 else "below" if nt < c else "equal" if nt == c else "above")
    for name in ("ecm_conv3d_wgrad_scratch_bytes", "ecm_conv_wino_wgrad_scratch_bytes", "ecm_conv2d_wgrad_ex_scratch_bytes"):
        assert seen[name] == {"zero", "answer", "clamp", "below", "equal", "above"}, (name, seen[name])
    assert seen["ecm_conv3d_c1_wgrad_scratch_bytes"] == {"zero", "answer", "below", "equal", "above"}
    assert seen["ecm_conv2d_c1_wgrad_scratch_bytes"] == {"zero", "answer"}


def test_every_query_equals_the_restated_plan(lib_mod):
    wrong = [(name, args, want, got) for name, args, want, _ in grid() for got in (lib_mod.query(name, *args),) if got != want]
    assert not wrong, f"{len(wrong)} of the grid differ, the first: {wrong[:5]}"


def test_scratch_is_refused_before_the_gpu(lib_mod):
    """ECM_ESCRATCH (-3) one byte short of the query, ECM_EUNSUP (-2) ahead of it: both answered without touching a GPU."""
    lib, one = lib_mod.load(), 16            # non-null addresses that are never dereferenced: every call returns before a launch
    q = lib_mod.query
    assert lib.ecm_conv3d_k3_wgrad(one, one, one, one, q("ecm_conv3d_wgrad_scratch_bytes", 1, 64, 64, 6, 32, 96, 1) - 1, 1, 64, 64, 6, 32, 96, 1, None) == -3
    assert lib.ecm_conv3d_k3_wgrad(one, one, one, one, 0, 1, 64, 64, 6, 32, 96, 3, None) == -2
    assert lib.ecm_conv_wino_wgrad(one, one, one, one, q("ecm_conv_wino_wgrad_scratch_bytes", 1, 64, 64, 6, 32, 96, 3) - 1, 1, 64, 64, 6, 32, 96, 3, None) == -3
    assert lib.ecm_conv_wino_wgrad(one, one, one, one, 0, 1, 64, 64, 6, 32, 96, 2, None) == -2
    nb = q("ecm_conv2d_wgrad_ex_scratch_bytes", 1, 64, 64, 32, 96, 3, 3, 1)
    assert lib.ecm_conv2d_wgrad_ex(one, one, one, one, nb - 1, 1, 64, 64, 32, 96, 3, 3, 1, 1, 1, 1, 32, 96, None) == -3
    # outside the table: short scratch is still reported first, enough scratch meets "no such kernel"
    nb = q("ecm_conv2d_wgrad_ex_scratch_bytes", 1, 64, 64, 32, 96, 5, 5, 1)
    assert lib.ecm_conv2d_wgrad_ex(one, one, one, one, nb - 1, 1, 64, 64, 32, 96, 5, 5, 1, 1, 2, 2, 32, 96, None) == -3
    assert lib.ecm_conv2d_wgrad_ex(one, one, one, one, nb, 1, 64, 64, 32, 96, 5, 5, 1, 1, 2, 2, 32, 96, None) == -2
    assert lib.ecm_conv2d_wgrad_ex(one, one, one, one, 1 << 40, 1, 64, 64, 32, 96, 3, 3, 1, 3, 1, 1, 32, 96, None) == -2      # dilation 3
    assert lib.ecm_conv3d_c1_wgrad(one, one, one, one, q("ecm_conv3d_c1_wgrad_scratch_bytes", 2, 32, 6, 9, 33) - 1, 2, 32, 6, 9, 33, None) == -3
    assert lib.ecm_conv3d_c1_wgrad(one, one, one, one, 1 << 40, 2, 33, 6, 9, 33, None) == -2
    assert lib.ecm_conv3d_c1_gn_wgrad(one, one, one, one, one, one, one, q("ecm_conv3d_c1_wgrad_scratch_bytes", 2, 32, 6, 9, 33) - 1, 2, 32, 6, 9, 33, None) == -3
    assert lib.ecm_conv2d_c1_wgrad(one, one, one, one, one, one, q("ecm_conv2d_c1_wgrad_scratch_bytes", 2, 32, 40, 70) - 1, 2, 32, 40, 70, None) == -3
