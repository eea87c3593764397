"""The KITTI training transform on the device: ops.color_jitter against Pillow's own bytes
(tests/golden/g13_jitter.npz), ops.frame_prep_jitter against color_jitter on the crops followed by the loader's five fp32
statements on the CPU, bit for bit, and the feeder's `jitter` keyword.  The numpy restatement (tests/jitter_restatement.py, held to
Pillow by tests/test_color_jitter_cpu.py) is only computed to name a difference."""
import ctypes as C
import hashlib
import importlib
import itertools
import os
import random

import numpy as np
import pytest
import torch

import jitter_restatement as R
from conftest import GOLDEN
from frame_fixtures import MEAN, STD, loader_statements, packed_shard as packed

pytestmark = pytest.mark.gpu

S = importlib.import_module("explicit-context-mapping-for-stereo-matching_amd.shards")
ESCRATCH = -3


@pytest.fixture(scope="module")
def ops():
    import ecm_amd
    assert torch.cuda.is_available(), "needs the MI355X"
    return ecm_amd.ops


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g13_jitter.npz")) as z:
        return {k: z[k] for k in z.files}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def first_difference(got, want):
    at = np.argwhere(got != want)
    return f"{len(at)} bytes differ, the first at {tuple(at[0])}: got {got[tuple(at[0])]}, want {want[tuple(at[0])]}" if len(at) else "equal"


def run(ops, img, rows):
    """color_jitter of the same image under rows = [(factors, order, shift)]: uint8 [len(rows),H,W,3] on the host."""
    x = torch.from_numpy(np.ascontiguousarray(img)).cuda().unsqueeze(0).repeat(len(rows), 1, 1, 1)
    pad = lambda o: list(o) + [-1] * (4 - len(o))                          # noqa: E731
    return ops.color_jitter(x, [list(r[0]) for r in rows], [pad(r[1]) for r in rows], [r[2] for r in rows]).cpu().numpy()


# ---- (a) Pillow, byte for byte --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "large"])       # 37x53 sits inside one reduction tile, 70x131 spans five with a ragged last one
def test_color_jitter_is_pillow_on_all_24_orders_and_every_single_operation(ops, golden, name):
    img = golden[f"{name}_image"]
    tile = ops.jitter_tile()
    assert (img.shape[0] * img.shape[1] <= tile) == (name == "small") and (name == "small" or img.shape[0] * img.shape[1] % tile)
    factors, shift = tuple(golden["factors"]), int(golden["shift"])
    orders = [tuple(int(c) for c in o) for o in golden["orders"]]
    assert sorted(orders) == sorted(itertools.permutations(range(4)))
    rows = [(factors, o, shift) for o in orders]
    want = list(golden[f"{name}_order_sha"])
    for code in range(3):
        for f, digest in zip(golden["single_factors"], golden[f"{name}_single_sha"][code]):
            rows.append(((f, f, f), (code,), 0))
            want.append(digest)
    for s, digest in zip(golden["single_shifts"], golden[f"{name}_hue_sha"]):
        rows.append((factors, (3,), int(s)))
        want.append(digest)
    assert len(rows) == 45
    got = run(ops, img, rows)
    for g, row, digest in zip(got, rows, want):
        if sha(g) != digest:
            pytest.fail(f"{name} {row}: {first_difference(g, R.jitter(img, *row))} (against the restatement)")
    if name == "small":
        for o, full in zip(golden["full_orders"], golden["small_full"]):
            assert np.array_equal(got[orders.index(tuple(int(c) for c in o))], full)


# ---- (b) all 2^24 colours through the hue round trip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_hue_round_trip_is_pillow_on_all_colours(ops, golden, k):
    shift, digest = int(golden["all_colours_shifts"][k]), str(golden["all_colours_hue_sha"][k])
    c = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
    img = torch.stack([c >> 16, (c >> 8) & 255, c & 255], -1).to(torch.uint8).reshape(1, 4096, 4096, 3)
    got = ops.color_jitter(img, [[1.0, 1.0, 1.0]], [[3, -1, -1, -1]], [shift]).cpu().numpy()[0]
    if sha(got) != digest:                                                   # only now the restatement, to name the colour
        for y in range(0, 4096, 256):
            want = R.hue(img[0, y:y + 256].cpu().numpy(), shift)
            if not np.array_equal(got[y:y + 256], want):
                pytest.fail(f"shift {shift}, rows {y}..: {first_difference(got[y:y + 256], want)}")
        pytest.fail(f"shift {shift}: the digest differs although the restatement agrees: the restatement is not Pillow's")


# ---- (c) the contrast mean at k + 0.5 and one count below -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", [False, True])
def test_contrast_mean_rounds_half_up_across_tiles(ops, prefix):
    H, W, k = 70, 131, 100
    n = H * W
    assert n % 2 == 0 and n > 4 * ops.jitter_tile()
    scale = 2 if prefix else 1                                              # brightness 0.5 in front halves 200 / 202 to 100 / 101
    for ones, m in ((n // 2, k + 1), (n // 2 - 1, k)):                      # mean gray exactly k + 0.5 -> k + 1; one count below -> k
        g = np.full(n, k * scale, np.uint8)
        g[n - ones:] = (k + 1) * scale                                      # the upper half lies in the last tiles, the ragged one among them
        img = np.repeat(g.reshape(H, W, 1), 3, 2)
        order = (0, 1) if prefix else (1,)
        got = run(ops, img, [((0.5, 0.0, 1.0), order, 0), ((0.5, 0.5, 1.0), order, 0), ((0.5, 1.4, 1.0), order, 0)])
        assert (got[0] == m).all(), (ones, np.unique(got[0]))               # factor 0: the image IS the mean
        for i, f in enumerate((0.0, 0.5, 1.4)):
            want = R.jitter(img, (0.5, f, 1.0), order, 0)
            assert np.array_equal(got[i], want), (ones, f, first_difference(got[i], want))


# ---- (d), (e) the decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [True, False])
def test_frame_prep_jitter_is_color_jitter_then_the_loader_statements(ops, half):
    B, H, W, th, tw = 3, 75, 140, 70, 131
    rgb, dsp = packed(B, H, W, half, 11)
    ys, xs = [5, 0, 2], [9, 0, 3]                                           # the first window touches the frame's last row and column
    p = ops.jitter_params(B, random.Random(3), torch.Generator().manual_seed(4))
    p.order = torch.tensor([[[0, 1, 2, 3], [3, 1, 0, 2]], [[2, 3, 1, 0], [1, -1, -1, -1]], [[3, 2, -1, -1], [-1, -1, -1, -1]]], dtype=torch.int32)
    p.pca[0, 0] = torch.tensor([0.9, -0.9, 0.02])                            # both clamps bind
    left, right, disp, image = ops.frame_prep_jitter((rgb.cuda(), dsp.cuda()), ys, xs, th, tw, p, want_image=True)
    views = torch.stack([rgb[b, ys[b]:ys[b] + th, xs[b]:xs[b] + tw, 3 * v:3 * v + 3] for b in range(B) for v in range(2)])
    u8 = ops.color_jitter(views.cuda(), p.factors.reshape(-1, 3), p.order.reshape(-1, 4), p.hue_shift.reshape(-1)).cpu()
    for b in range(B):
        for v, got in enumerate((left, right)):
            img, want = loader_statements(u8[2 * b + v], p.pca[b, v])
            assert torch.equal(got[b].cpu(), want), (b, v, (got[b].cpu() - want).abs().max())
            if v == 0:
                assert torch.equal(image[b].cpu(), img) and 0 <= float(img.min()) and float(img.max()) <= 1
        assert torch.equal(disp[b].cpu(), dsp[b, ys[b]:ys[b] + th, xs[b]:xs[b] + tw].float())
    assert float(image[0, 0].max()) == 1.0 and float(image[0, 1].min()) == 0.0
    three = ops.frame_prep_jitter((rgb.cuda(), dsp.cuda()), ys, xs, th, tw, p)
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, (left, right, disp)))


def no_jitter(ops, B):
    p = ops.jitter_params(B, random.Random(0), torch.Generator(), brightness=0, contrast=0, saturation=0, hue=0, alphastd=0)
    assert (p.order == -1).all() and (p.pca == 0).all() and (p.hue_shift == 0).all()
    return p


@pytest.mark.parametrize("half", [True, False])
def test_no_operations_and_no_shift_is_frame_prep(ops, half):
    B, H, W, th, tw = 2, 50, 70, 47, 64
    rgb, dsp = packed(B, H, W, half, 12)
    frames = (rgb.cuda(), dsp.cuda())
    ys, xs = [3, 0], [6, 1]
    got = ops.frame_prep_jitter(frames, ys, xs, th, tw, no_jitter(ops, B))
    want = ops.frame_prep(frames, ys, xs, th, tw)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


# ---- (f) guard bands ------------------------------------------------------------------------------------------------------------------------
def test_outputs_and_scratch_stay_inside_their_buffers(ops):
    import ecm_amd
    lib = ecm_amd._lib
    B, H, W, th, tw = 2, 75, 140, 70, 131
    rgb, dsp = packed(B, H, W, True, 13)
    rgb, dsp = rgb.cuda(), dsp.cuda()
    p = ops.jitter_params(B, random.Random(5), torch.Generator().manual_seed(6))
    nbytes = lib.query("ecma_jitter_scratch_bytes", 2 * B, th, tw)
    assert nbytes == 2 * B * -(-th * tw // ops.jitter_tile()) * 4
    G = 4096
    sizes = dict(left=B * 3 * th * tw * 4, right=B * 3 * th * tw * 4, disp=B * th * tw * 4, image=B * 3 * th * tw * 4, scratch=nbytes)
    bufs = {k: torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
    ptr = {k: C.c_void_p(b.data_ptr() + G) for k, b in bufs.items()}
    host = lambda t, v: C.cast((t * len(v))(*v), C.c_void_p)                 # noqa: E731
    args = lambda scratch_bytes: (                                           # noqa: E731
        C.c_void_p(rgb.data_ptr()), C.c_void_p(dsp.data_ptr()), 1, ptr["left"], ptr["right"], ptr["disp"], ptr["image"], B, H, W,
        host(C.c_int, [5, 0]), host(C.c_int, [9, 2]), th, tw, host(C.c_float, p.factors.reshape(-1).tolist()),
        host(C.c_int, p.order.reshape(-1).tolist()), host(C.c_int, p.hue_shift.reshape(-1).tolist()),
        host(C.c_float, p.pca.reshape(-1).tolist()), host(C.c_float, MEAN), host(C.c_float, STD), ptr["scratch"],
        C.c_longlong(scratch_bytes), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert lib.load().ecma_frame_prep_jitter_fwd(*args(nbytes - 1)) == ESCRATCH          # one byte short: refused, nothing launched
    torch.cuda.synchronize()
    assert all(bool((b == 0xA5).all()) for b in bufs.values())
    lib.call("ecma_frame_prep_jitter_fwd", *args(nbytes))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[:G] == 0xA5).all()) and bool((b[-G:] == 0xA5).all()), k
    want = ops.frame_prep_jitter((rgb, dsp), [5, 0], [9, 2], th, tw, p, want_image=True)
    for k, w in zip(("left", "right", "disp", "image"), want):
        assert torch.equal(bufs[k][G:-G].view(torch.float32).reshape(w.shape), w), k
    # the uint8 op: output and scratch
    x = rgb[:, :, :, :3].contiguous()
    n1 = lib.query("ecma_jitter_scratch_bytes", B, H, W)
    out, scr = (torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for n in (x.numel(), n1))
    a = lambda scratch_bytes: (C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr() + G), B, H, W,      # noqa: E731
                               host(C.c_float, p.factors[:, 0].reshape(-1).tolist()), host(C.c_int, p.order[:, 0].reshape(-1).tolist()),
                               host(C.c_int, p.hue_shift[:, 0].tolist()), C.c_void_p(scr.data_ptr() + G), C.c_longlong(scratch_bytes),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert lib.load().ecma_color_jitter_fwd(*a(n1 - 1)) == ESCRATCH
    lib.call("ecma_color_jitter_fwd", *a(n1))
    torch.cuda.synchronize()
    for b in (out, scr):
        assert bool((b[:G] == 0xA5).all()) and bool((b[-G:] == 0xA5).all())
    assert torch.equal(out[G:-G].reshape(x.shape), ops.color_jitter(x, p.factors[:, 0], p.order[:, 0], p.hue_shift[:, 0]))


# ---- (g) the feeder -------------------------------------------------------------------------------------------------------------------------
def test_feeder_jitter_repeats_replays_and_none_is_the_old_path(ops, tmp_path):
    rs = np.random.RandomState(7)
    frames = [np.concatenate([rs.randint(0, 256, (40, 60, 6)).astype(np.float32), rs.rand(40, 60, 1).astype(np.float32) * 90], 2)
              for _ in range(6)]
    reader = S.ShardReader(S.write_shard(frames, str(tmp_path / "s.ecms"), "fp32"))
    make = lambda jitter: S.ShardFeeder(reader, batch=2, split="train", seed=9, crop=(32, 48), want_image=True, jitter=jitter)   # noqa: E731
    a, b, plain = make(dict(ops.KITTI_JITTER)), make(dict(ops.KITTI_JITTER)), make(None)
    assert a.last_jitter is None
    seen = []
    for epoch in range(2):
        for (ba, bb, bp) in zip(iter(a), iter(b), iter(plain)):
            assert all(torch.equal(x, y) for x, y in zip(ba, bb))                              # the same seed: the same batches
            assert a.last_indices == b.last_indices == plain.last_indices and a.last_windows == b.last_windows == plain.last_windows
            p = a.last_jitter
            assert plain.last_jitter is None and all(torch.equal(getattr(p, f), getattr(b.last_jitter, f)) for f in ("factors", "order", "hue_shift", "pca"))
            crops = [reader.frame(i) for i in a.last_indices]
            rgb = torch.stack([torch.from_numpy(np.array(c[0][y:y + 32, x:x + 48])) for c, (y, x) in zip(crops, a.last_windows)]).cuda()
            dsp = torch.stack([torch.from_numpy(np.array(c[1][y:y + 32, x:x + 48])) for c, (y, x) in zip(crops, a.last_windows)]).cuda()
            replay = ops.frame_prep_jitter((rgb, dsp), [0, 0], [0, 0], 32, 48, p, want_image=True)
            assert all(torch.equal(x, y) for x, y in zip(ba, replay))                          # last_jitter replayed reproduces the batch
            old = ops.frame_prep((rgb, dsp), [0, 0], [0, 0], 32, 48, want_image=True)
            assert all(torch.equal(x, y) for x, y in zip(bp, old))                             # jitter=None: today's path, bit for bit
            assert torch.equal(ba[2], bp[2]) and not torch.equal(ba[0], bp[0])
            seen.append(p)
    assert len(seen) == 6 and not torch.equal(seen[0].factors, seen[3].factors)                # a new epoch draws anew
    for f in (a, b, plain):
        f.close()
