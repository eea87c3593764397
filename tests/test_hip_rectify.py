"""ops.rectify_map, ops.remap_pair and models.StereoRig on the device against rectify_map_t and remap_t of
tests/test_rectify_cpu.py.

The map: the device evaluates the header's fp64 expression operation for operation, so bit-equality with the restatement rounded
to fp32 is expected and counted; the bound is |got - want64| <= ulp32(max(|want64|, 1)).
The remap, on GIVEN maps (map rounding plays no part): masks exact; on integer-coordinate maps the planes are bit-equal to the
fp32 restatement (and, for uint8 frames under the identity, to ops.frame_prep on the same packed shard); on sub-pixel maps the
distance from the fp64 restatement may be at most 4x the largest distance of the fp32 restatement of the same formula from fp64 on
that fixture -- both are printed.
The shapes are the smallest at which an index can go wrong: one pixel, widths around the 4-pixel vector store (1, 3, 4, 5, 8), the
workgroup's extent (64 x 16) and one more or less, output sizes that differ from the source's, several images."""
import ctypes as C

import pytest
import torch

from test_rectify_cpu import MEAN, STD, frames, integer_map, rectify_map_t, remap_t, rig
import test_hip_abi_calls as abi_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
F64 = torch.float64


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def TILE(ecm):
    return ecm.ops.rectify_tile_width()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- the map ------------------------------------------------------------------------------------------------------------------------
EXACT = {"cases": 0, "entries": 0, "not_bit_equal": 0}


def map_sizes(TILE):
    return {"one_pixel": (1, 1), "small": (3, 5), "tile_minus": (2, TILE - 1), "tile": (2, TILE), "tile_plus": (2, TILE + 1)}


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "aligned"])
@pytest.mark.parametrize("n", [4, 5, 8])
@pytest.mark.parametrize("size", ["one_pixel", "small", "tile_minus", "tile", "tile_plus"])
def test_rectify_map(ecm, TILE, size, n, rotated):
    Ho, Wo = map_sizes(TILE)[size]
    K1, D1, K2, D2, R, T, raw_size = rig(n, rotated=rotated)
    r = ecm.ops.stereo_rectify(K1, D1, K2, D2, R, T, raw_size, new_size=(Ho, Wo), focal=80.0, center=(0.47 * Wo + 0.3, 0.45 * Ho + 0.2))
    for K, D, Rn, Pn in ((K1, D1, r.R1, r.P1), (K2, D2, r.R2, r.P2)):
        want32, want64 = rectify_map_t(K, D, Rn, Pn, (Ho, Wo))
        got = ecm.ops.rectify_map(K, D, Rn, Pn, (Ho, Wo), DEV)
        assert got.shape == (2, Ho, Wo) and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
        got = got.cpu()
        assert bool(torch.isfinite(got).all())
        ulp = torch.exp2(torch.floor(torch.log2(want64.abs().clamp(min=1.0))) - 23)
        off = (got.to(F64) - want64).abs()
        EXACT["cases"] += 1
        EXACT["entries"] += got.numel()
        EXACT["not_bit_equal"] += int((bits(got) != bits(want32)).sum())
        assert bool((off <= ulp).all()), float((off / ulp).max())


def test_the_map_was_bit_equal():
    """Runs after the cases above: how many entries were not bit-equal to the restatement (the bound stays one ulp either way)."""
    print(f"RECTIFY_MAP {EXACT['cases']} maps, {EXACT['entries']} entries, {EXACT['not_bit_equal']} not bit-equal to the fp64 restatement")
    assert EXACT["cases"] > 0


# ---- the remap ----------------------------------------------------------------------------------------------------------------------
def boundary(W):
    return [-1.0, -2.0 ** -10, 0.0, W - 2.0, W - 1.0, W - 1 + 2.0 ** -10, float(W), NAN, INF, -INF, 1e30, -1e30]


def subpixel_map(B, H, W, Ho, Wo, seed):
    """[B,2,Ho,Wo] (B = 0: [2,Ho,Wo]): random coordinates from 1.5 px outside the source on every side, then -- as far as they fit --
    the boundary coordinates along x at row 1 and along y at column 1."""
    g = torch.Generator().manual_seed(seed)
    n = max(B, 1)
    mx = torch.rand(n, Ho * Wo, generator=g) * (W + 2.0) - 1.5
    my = torch.rand(n, Ho * Wo, generator=g) * (H + 2.0) - 1.5
    bx, by = torch.tensor(boundary(W)), torch.tensor(boundary(H))
    k = min(len(bx), Ho * Wo // 2)
    mx[:, :k], my[:, :k] = bx[:k], 1.0
    mx[:, k:2 * k], my[:, k:2 * k] = 1.0, by[:k]
    m = torch.stack([mx, my], 1).view(n, 2, Ho, Wo).to(torch.float32)
    return m if B else m[0].contiguous()


def run_remap(ecm, left, right, ml, mr, **kw):
    dev = lambda t: t.to(DEV)                                                               # noqa: E731
    return tuple(t.cpu() for t in ecm.ops.remap_pair(dev(left), dev(right), dev(ml), dev(mr), want_image=True, with_mask=True, **kw))


WORST = {"kernel": 0.0, "fp32": 0.0}

REMAP_SHAPES = {"5x7_to_3x5": ((5, 7), (3, 5)), "to_tile_minus": ((9, 19), (17, 63)), "to_tile": ((9, 19), (16, 64)),
                "to_tile_plus": ((9, 19), (15, 65)), "w1": ((9, 19), (2, 1)), "w3": ((9, 19), (2, 3)), "w4": ((9, 19), (2, 4)),
                "w8": ((9, 19), (3, 8))}


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("shape", list(REMAP_SHAPES))
def test_remap_subpixel(ecm, shape, kind):
    (H, W), (Ho, Wo) = REMAP_SHAPES[shape]
    for B, per_image in ((1, False), (3, False), (3, True), (1, True)):
        left, right = frames(B, H, W, 10 + B, kind), frames(B, H, W, 20 + B, kind)
        ml = subpixel_map(B if per_image else 0, H, W, Ho, Wo, 30 + Wo)
        mr = subpixel_map(B if per_image else 0, H, W, Ho, Wo, 40 + Wo)
        got_l, got_r, got_image, got_kl, got_kr = run_remap(ecm, left, right, ml, mr, border=23.0)
        for raw, mp, got, mask, image in ((left, ml, got_l, got_kl, got_image), (right, mr, got_r, got_kr, None)):
            want64, image64, want_mask = remap_t(raw, mp, border=23.0)
            want32, image32, _ = remap_t(raw, mp, border=23.0, dtype=torch.float32)
            assert got.shape == (B, 3, Ho, Wo) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
            assert mask.dtype == torch.bool and torch.equal(mask, want_mask)                # exact
            kernel, fp32 = float((got.to(F64) - want64).abs().max()), float((want32.to(F64) - want64).abs().max())
            WORST["kernel"], WORST["fp32"] = max(WORST["kernel"], kernel), max(WORST["fp32"], fp32)
            print(f"REMAP {shape} {kind} B={B} per_image={per_image}: kernel {kernel:.3e}, fp32 restatement {fp32:.3e} from fp64")
            assert fp32 > 0 and kernel <= 4 * fp32
            if image is not None:
                kernel_i, fp32_i = float((image.to(F64) - image64).abs().max()), float((image32.to(F64) - image64).abs().max())
                assert kernel_i <= 4 * fp32_i
        assert bool(got_kl.any()) or Ho * Wo < 4


def test_the_remap_distances():
    print(f"REMAP worst distance from fp64: kernel {WORST['kernel']:.3e}, fp32 restatement {WORST['fp32']:.3e}")
    assert WORST["fp32"] > 0


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("shape", list(REMAP_SHAPES))
def test_remap_integer_maps_are_bit_equal(ecm, shape, kind):
    (H, W), (Ho, Wo) = REMAP_SHAPES[shape]
    B = 3
    left, right = frames(B, H, W, 50, kind), frames(B, H, W, 51, kind)
    ml, mr = integer_map(Ho, Wo, dx=-2, dy=1), torch.stack([integer_map(Ho, Wo, dx=b - 1, dy=-b) for b in range(B)])
    mr = mr if shape != "w4" else mr[0].contiguous()
    if mr.dim() == 4:
        ml = ml.unsqueeze(0).expand(B, -1, -1, -1).contiguous()
    got_l, got_r, got_image, got_kl, got_kr = run_remap(ecm, left, right, ml, mr, border=200.0)
    for raw, mp, got, mask in ((left, ml, got_l, got_kl), (right, mr, got_r, got_kr)):
        want, image, want_mask = remap_t(raw, mp, border=200.0, dtype=torch.float32)
        assert same(got, want) and torch.equal(mask, want_mask)
        if raw is left:
            assert same(got_image, image)


@pytest.mark.parametrize("H,W", [(5, 7), (16, 64), (17, 65), (3, 8)])
def test_identity_map_is_frame_prep_bit_for_bit(ecm, H, W):
    B = 2
    left, right = frames(B, H, W, 60), frames(B, H, W, 61)
    shard = (torch.cat([left, right], -1).to(DEV), torch.zeros(B, H, W, device=DEV))
    want_l, want_r, _ = ecm.ops.frame_prep(shard, [0] * B, [0] * B, H, W)
    ident = integer_map(H, W).to(DEV)
    got = ecm.ops.remap_pair(left.to(DEV), right.to(DEV), ident, ident, with_mask=True)
    assert len(got) == 4 and same(got[0], want_l) and same(got[1], want_r)
    inside = torch.zeros(B, H, W, dtype=torch.bool)
    inside[:, :H - 1, :W - 1] = True
    assert torch.equal(got[2].cpu(), inside) and torch.equal(got[3].cpu(), inside)
    plain = ecm.ops.remap_pair(left.to(DEV), right.to(DEV), ident, ident)
    assert len(plain) == 2 and same(plain[0], want_l) and same(plain[1], want_r)
    with_image = ecm.ops.remap_pair(left.to(DEV), right.to(DEV), ident, ident, want_image=True)
    assert len(with_image) == 3 and same(with_image[2].cpu(), left.permute(0, 3, 1, 2).to(torch.float32) / 255.0)


def test_other_normalisations_and_a_view_as_input(ecm):
    H, W, Ho, Wo = 9, 19, 6, 12
    left, right = frames(2, H, W + 3, 70, "f32")[..., 2:W + 2], frames(2, H, W, 71, "f32")   # a non-contiguous view
    mp = subpixel_map(0, H, W, Ho, Wo, 72)
    mean, std = (0.1, 0.2, 0.3), (0.5, 0.25, 2.0)
    got = ecm.ops.remap_pair(left.to(DEV)[..., :], right.to(DEV), mp.to(DEV), mp.to(DEV), mean=mean, std=std, border=-4.0)
    for raw, g in ((left, got[0]), (right, got[1])):
        want64 = remap_t(raw.contiguous(), mp, mean, std, -4.0)[0]
        want32 = remap_t(raw.contiguous(), mp, mean, std, -4.0, dtype=torch.float32)[0]
        assert float((g.cpu().to(F64) - want64).abs().max()) <= 4 * float((want32.to(F64) - want64).abs().max())


# ---- properties ---------------------------------------------------------------------------------------------------------------------
def _case(B=3, H=9, W=19, Ho=17, Wo=65, kind="u8"):
    return (frames(B, H, W, 80, kind).to(DEV), frames(B, H, W, 81, kind).to(DEV), subpixel_map(B, H, W, Ho, Wo, 82).to(DEV),
            subpixel_map(B, H, W, Ho, Wo, 83).to(DEV))


@pytest.mark.parametrize("Wo", [64, 65])
def test_guard_bands(ecm, Wo):
    """Through the ABI directly, on canary-filled buffers: nothing is written after any output, on the vector path (Wo = 64) and
    on the scalar one."""
    lib = ecm._lib
    B, H, W, Ho, BAND, CANARY = 3, 9, 19, 17, 4096, 0xA5
    left, right, ml, mr = _case(B, H, W, Ho, Wo)
    n = B * Ho * Wo
    sizes = {"left": n * 12, "right": n * 12, "image": n * 12, "mask_l": n, "mask_r": n}
    bufs = {k: torch.full((v + BAND,), CANARY, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    p = lambda t: C.c_void_p(t.data_ptr())                                                  # noqa: E731
    host = lambda v: C.cast((C.c_float * 3)(*v), C.c_void_p)                                # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.call("ecmr_remap_pair_fwd", p(left), p(right), 1, p(ml), p(mr), 1, p(bufs["left"]), p(bufs["right"]), p(bufs["image"]),
             p(bufs["mask_l"]), p(bufs["mask_r"]), B, H, W, Ho, Wo, host(MEAN), host(STD), 0.0, st)
    ecm.ops.check_async_errors()
    for k, size in sizes.items():
        assert bool((bufs[k][size:] == CANARY).all()), k
    want = ecm.ops.remap_pair(left, right, ml, mr, want_image=True, with_mask=True)
    for k, w in zip(sizes, want):
        assert torch.equal(bufs[k][:sizes[k]], w.contiguous().view(-1).view(torch.uint8)), k
    # the map entry, the same way
    K1, D1, _, _, R, T, size = rig()
    r = ecm.ops.stereo_rectify(K1, D1, K1, D1, R, T, size, new_size=(3, Wo))
    params = ecm.ops.rectify_map_params(K1, D1, r.R1, r.P1).to(DEV)
    out = torch.full((2 * 3 * Wo * 4 + BAND,), CANARY, dtype=torch.uint8, device=DEV)
    lib.call("ecmr_rectify_map_fwd", p(params), p(out), 3, Wo, st)
    ecm.ops.check_async_errors()
    assert bool((out[2 * 3 * Wo * 4:] == CANARY).all())
    assert torch.equal(out[:2 * 3 * Wo * 4].view(torch.float32).view(2, 3, Wo), ecm.ops.rectify_map(K1, D1, r.R1, r.P1, (3, Wo), DEV))


def test_runs_on_the_current_stream_and_twice_the_same(ecm):
    left, right, ml, mr = _case()
    first = ecm.ops.remap_pair(left, right, ml, mr, want_image=True, with_mask=True)
    again = ecm.ops.remap_pair(left, right, ml, mr, want_image=True, with_mask=True)
    assert all(same(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        on_side = ecm.ops.remap_pair(left, right, ml, mr, want_image=True, with_mask=True)
        K1, D1, _, _, R, T, size = rig()
        r = ecm.ops.stereo_rectify(K1, D1, K1, D1, R, T, size)
        side_map = ecm.ops.rectify_map(K1, D1, r.R1, r.P1, size, DEV)
    side.synchronize()
    ecm.ops.check_async_errors()
    assert all(same(a, b) for a, b in zip(first, on_side))
    assert same(side_map, ecm.ops.rectify_map(K1, D1, r.R1, r.P1, size, DEV))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_an_image_does_not_depend_on_the_rest_of_the_batch(ecm, kind):
    left, right, ml, mr = _case(kind=kind)
    whole = ecm.ops.remap_pair(left, right, ml, mr, want_image=True, with_mask=True)
    for b in range(left.shape[0]):
        one = ecm.ops.remap_pair(left[b:b + 1], right[b:b + 1], ml[b:b + 1], mr[b:b + 1], want_image=True, with_mask=True)
        assert all(same(o, w[b:b + 1]) for o, w in zip(one, whole))
    other = left.clone()
    other[1:] = 255 - other[1:]                                                           # the other images change, image 0 does not
    changed = ecm.ops.remap_pair(other, right, ml, mr, want_image=True, with_mask=True)
    assert all(same(c[:1], w[:1]) for c, w in zip(changed, whole)) and not same(changed[0], whole[0])


# ---- what ops.py hands to the third table ------------------------------------------------------------------------------------------
def test_every_rectify_prototype_is_called_with_well_typed_arguments(ecm):
    left, right, ml, mr = _case()
    K1, D1, K2, D2, R, T, size = rig(8)
    r = ecm.ops.stereo_rectify(K1, D1, K2, D2, R, T, size)
    with abi_calls.recording(ecm, "rectify", ecm._lib.RECTIFY_PROTOTYPES) as calls:
        ecm.ops.rectify_tile_width()
        ecm.ops.rectify_map(K2, D2, r.R2, r.P2, (5, 9), DEV)
        ecm.ops.remap_pair(left, right, ml, mr, want_image=True, with_mask=True)
        ecm.ops.remap_pair(left, right, ml[0], mr[0], border=3)                             # an int border, shared maps
        ecm.ops.remap_pair(left, right, ml[:, :, :, 1:], mr[:, :, :, 1:])                   # views: made contiguous and aligned
        f32 = left.permute(0, 3, 1, 2).float()
        ecm.ops.remap_pair(f32, f32.contiguous(), ml, mr, with_mask=True)                   # a permuted fp32 source
    assert set(calls) == set(ecm._lib.RECTIFY_PROTOTYPES), sorted(set(ecm._lib.RECTIFY_PROTOTYPES) - set(calls))
    assert not set(abi_calls.INT_MAX) & set(ecm._lib.RECTIFY_PROTOTYPES)


# ---- the rig ------------------------------------------------------------------------------------------------------------------------
_models = {}


def _model(ecm, arch):
    if arch not in _models:
        torch.manual_seed(5)
        _models[arch] = ecm.get_model(arch).to(DEV).eval()
    return _models[arch]


def _rig(ecm, new_size):
    return ecm.models.StereoRig(*rig(5, size=(72, 96)), new_size=new_size)


def test_rig_is_the_ops_it_wraps(ecm):
    sr = _rig(ecm, (40, 52))
    K1, D1, K2, D2, R, T, size = rig(5, size=(72, 96))
    maps = sr.maps(DEV)
    assert sr.maps(torch.device(DEV, torch.cuda.current_device()))[0] is maps[0] and sr.maps(DEV)[1] is maps[1]   # computed once
    r = sr.rectification
    assert same(maps[0], ecm.ops.rectify_map(K1, D1, r.R1, r.P1, (40, 52), DEV))
    assert same(maps[1], ecm.ops.rectify_map(K2, D2, r.R2, r.P2, (40, 52), DEV))
    for kind in ("u8", "f32"):
        left, right = frames(2, 72, 96, 90, kind).to(DEV), frames(2, 72, 96, 91, kind).to(DEV)
        for kw in ({}, {"want_image": True}, {"with_mask": True}, {"want_image": True, "with_mask": True}):
            got, want = sr(left, right, **kw), ecm.ops.remap_pair(left, right, *maps, **kw)
            assert len(got) == len(want) == 2 + kw.get("want_image", 0) + 2 * kw.get("with_mask", 0)
            assert all(same(a, b) for a, b in zip(got, want))
    # the maps land inside the raw frame for most of the rectified one
    masks = sr(left, right, with_mask=True)[2:]
    assert all(float(m.float().mean()) > 0.5 for m in masks)


@pytest.mark.parametrize("source", ["forward", "smooth"])
def test_rig_point_cloud_is_the_models(ecm, source):
    model = _model(ecm, "cmfsm")
    K1, D1, K2, D2, R, T, _ = rig(5)
    sr = ecm.models.StereoRig(K1 * torch.tensor([[5.0], [5.0], [1.0]], dtype=F64), D1, K2 * torch.tensor([[5.0], [5.0], [1.0]], dtype=F64),
                              D2, R, T, (240, 320), new_size=(256, 256))
    g = torch.Generator().manual_seed(95)
    smooth = torch.nn.functional.interpolate(torch.rand(2, 3, 15, 20, generator=g), size=(240, 320), mode="bilinear") * 255
    left = smooth[:1].round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(DEV)
    right = smooth[1:].round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(DEV)
    with torch.no_grad():
        pc = sr.point_cloud(model, left, right, source=source)
        rect_l, rect_r, image = sr(left, right, want_image=True)
        want = model.point_cloud(rect_l, rect_r, sr.Q, colors=image, source=source)
    assert type(pc) is ecm.models.PointCloud and pc.points.shape[1] == 6 and pc.xyz.shape == (1, 3, 256, 256)
    for a, b in zip(pc[:4], want[:4]):
        assert same(a, b)
    assert all(same(a, b) for a, b in zip(tuple(pc.stage), tuple(want.stage)))
    if source == "forward":
        plain = sr.point_cloud(model, left, right, source="forward", colors=None)
        assert plain.points.shape == (len(pc.points), 3)
