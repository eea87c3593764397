"""The KITTI training transform without a GPU: the numpy restatement of include/ecm_augment.h
(tests/jitter_restatement.py) against the Pillow fixture tests/golden/g13_jitter.npz and, where Pillow imports, against Pillow
itself -- both conversions over all 2^24 inputs included; ops.jitter_params; the census of the ninth header, held as
tests/test_volume_color_cpu.py holds the eighth; its refusal contract with the devices hidden; and the Python refusals."""
import ctypes as C
import hashlib
import itertools
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_refusal_child as child
import jitter_restatement as R
from conftest import GOLDEN
from test_abi_refusals import EINVAL, ESCRATCH, EUNSUP, HIDE, Row, _report, calls_of, classify, classify_query, query_calls
from test_abi_types import INCLUDE, _strip, compare, lib_mod, package_entry_names, parse_header  # noqa: F401  (lib_mod: a fixture)

HEADER, PREFIX = "ecm_augment.h", "ecma_"
ENTRIES = ("ecma_jitter_tile", "ecma_jitter_scratch_bytes", "ecma_color_jitter_fwd", "ecma_frame_prep_jitter_fwd")
TILE = 2048


def ecm():
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g13_jitter.npz")) as z:
        return {k: z[k] for k in z.files}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c >> 16, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


# ---- the restatement against the fixture, without Pillow ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "large"])
def test_restatement_equals_the_fixture(golden, name):
    img = golden[f"{name}_image"]
    assert img.shape == {"small": (37, 53, 3), "large": (70, 131, 3)}[name] and img.dtype == np.uint8
    factors, shift = tuple(golden["factors"]), int(golden["shift"])
    orders = [tuple(int(c) for c in o) for o in golden["orders"]]
    assert sorted(orders) == sorted(itertools.permutations(range(4)))
    for o, digest in zip(orders, golden[f"{name}_order_sha"]):
        assert sha(R.jitter(img, factors, o, shift)) == digest, o
    assert tuple(golden["single_factors"]) == (0.0, 0.6, 0.83, 1.0, 1.17, 1.4) and tuple(golden["single_shifts"]) == (0, 77, 231)
    for code in range(3):
        for f, digest in zip(golden["single_factors"], golden[f"{name}_single_sha"][code]):
            assert sha(R.jitter(img, (f, f, f), (code,), 0)) == digest, (code, f)
    for s, digest in zip(golden["single_shifts"], golden[f"{name}_hue_sha"]):
        assert sha(R.jitter(img, factors, (3,), int(s))) == digest, s
    if name == "small":
        for o, full in zip(golden["full_orders"], golden["small_full"]):
            assert np.array_equal(R.jitter(img, factors, tuple(o), shift), full)
    assert len(set(golden[f"{name}_order_sha"])) == 24                       # the order matters: no two agree


def test_hue_round_trip_is_not_the_identity_and_the_sweep_digests_hold(golden):
    c = all_colours()
    for shift, digest in zip(golden["all_colours_shifts"], golden["all_colours_hue_sha"]):
        h = hashlib.sha256()
        same = 0
        for y in range(0, 4096, 512):
            out = R.hue(c[y:y + 512], int(shift))
            same += int((out == c[y:y + 512]).all(-1).sum())
            h.update(out.tobytes())
        assert h.hexdigest() == str(digest), shift
        assert same < (1 << 24)                                              # even at shift 0 some colours move
    assert os.path.getsize(os.path.join(GOLDEN, "g13_jitter.npz")) < 100 * 1024


# ---- the restatement against Pillow itself -----------------------------------------------------------------------------------------------
def pil_hue(Image, im, shift):
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(shift)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_jitter(img, factors, order, shift):
    from PIL import Image, ImageEnhance
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    im = Image.fromarray(img, "RGB")
    for code in order:
        im = pil_hue(Image, im, shift) if code == 3 else enh[code](im).enhance(factors[code])
    return np.array(im)


def test_restatement_equals_pillow_on_drawn_parameters(golden):
    pytest.importorskip("PIL")
    rng = random.Random(21)
    gen = torch.Generator().manual_seed(22)
    p = ecm().ops.jitter_params(12, rng, gen)
    for name in ("small", "large"):
        img = golden[f"{name}_image"]
        for b in range(12):
            f, o, s = p.factors[b, 0].tolist(), [c for c in p.order[b, 0].tolist() if c >= 0], int(p.hue_shift[b, 0])
            assert np.array_equal(R.jitter(img, f, o, s), pil_jitter(img, f, o, s)), (name, f, o, s)
    img = golden["small_image"]
    for f in (0.0, 0.25, 0.6, 1.0, 1.4, 1.9, 3.0):                          # beyond the drawn range: the clamped branch of the blend
        for code in range(3):
            assert np.array_equal(R.jitter(img, (f, f, f), (code,), 0), pil_jitter(img, (f, f, f), (code,), 0)), (code, f)


def test_both_conversions_equal_pillow_on_all_inputs():
    Image = pytest.importorskip("PIL.Image")
    c = all_colours()
    for y in range(0, 4096, 512):
        part = np.ascontiguousarray(c[y:y + 512])
        want = np.array(Image.fromarray(part, "RGB").convert("HSV"))
        got = R.rgb_to_hsv(part)
        assert np.array_equal(got, want), (y, np.argwhere(got != want)[:1])
        want = np.array(Image.fromarray(part, "HSV").convert("RGB"))          # the same 2^24 triples read as H, S, V
        got = R.hsv_to_rgb(part)
        assert np.array_equal(got, want), (y, np.argwhere(got != want)[:1])


def test_contrast_mean_is_imagestat_at_the_half_and_one_below():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageStat
    H, W = 70, 131
    n = H * W
    for k in (0, 100, 254):
        for ones, m in ((n // 2, k + 1), (n // 2 - 1, k)):
            g = np.full(n, k, np.uint8)
            g[n - ones:] = k + 1
            img = np.repeat(g.reshape(H, W, 1), 3, 2)
            assert np.array_equal(R.gray(img), g.reshape(H, W))
            assert int(ImageStat.Stat(Image.fromarray(img, "RGB").convert("L")).mean[0] + 0.5) == m == R.contrast_mean(img)
            assert (np.array(ImageEnhance.Contrast(Image.fromarray(img, "RGB")).enhance(0.0)) == m).all()
            assert (R.jitter(img, (1, 0.0, 1), (1,), 0) == m).all()
    rs = np.random.RandomState(3)
    for _ in range(20):
        img = rs.randint(0, 256, (rs.randint(1, 40), rs.randint(1, 40), 3)).astype(np.uint8)
        im = Image.fromarray(img, "RGB")
        assert np.array_equal(R.gray(img), np.array(im.convert("L")))
        assert R.contrast_mean(img) == int(ImageStat.Stat(im.convert("L")).mean[0] + 0.5)


# ---- jitter_params ---------------------------------------------------------------------------------------------------------------------
def draw(batch=64, seed=(1, 2), **kw):
    return ecm().ops.jitter_params(batch, random.Random(seed[0]), torch.Generator().manual_seed(seed[1]), **kw)


def test_jitter_params_ranges_permutations_and_repeatability():
    ops = ecm().ops
    assert ops.KITTI_JITTER == dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.4, alphastd=0.1)
    p = draw(**ops.KITTI_JITTER)
    assert p.factors.shape == (64, 2, 3) and p.order.shape == (64, 2, 4) and p.hue_shift.shape == (64, 2) and p.pca.shape == (64, 2, 3)
    assert p.factors.dtype == p.pca.dtype == torch.float32 and p.order.dtype == p.hue_shift.dtype == torch.int32
    assert float(p.factors.min()) >= 0.6 and float(p.factors.max()) <= 1.4 and float(p.factors.std()) > 0.1
    # uniform(-0.4, 0.4) * 255 truncated lies in -101..101: 0..101 and 155..255 after the uint8 wrap
    assert all(s <= 101 or s >= 155 for s in p.hue_shift.reshape(-1).tolist()) and len(set(p.hue_shift.reshape(-1).tolist())) > 30
    assert (p.order.sort(-1).values == torch.arange(4, dtype=torch.int32)).all()
    assert len({tuple(o) for o in p.order.reshape(-1, 4).tolist()}) >= 20    # of 24 orders, over 128 views
    assert not torch.equal(p.factors[:, 0], p.factors[:, 1]) and not torch.equal(p.order[:, 0], p.order[:, 1])       # the views draw on their own
    assert not torch.equal(p.pca[:, 0], p.pca[:, 1]) and not torch.equal(p.hue_shift[:, 0], p.hue_shift[:, 1])
    assert 0.003 < float(p.pca.abs().mean()) < 0.03                          # |eigvec . (alpha eigval)| at alphastd 0.1
    q = draw(**ops.KITTI_JITTER)
    assert all(torch.equal(getattr(p, f), getattr(q, f)) for f in ("factors", "order", "hue_shift", "pca"))
    r = draw(seed=(3, 2), **ops.KITTI_JITTER)
    assert not torch.equal(p.factors, r.factors) and torch.equal(p.pca, r.pca)       # the normals come from gen alone
    big = draw(brightness=1.5, contrast=0.1, saturation=0.4, hue=0.5)
    assert float(big.factors[..., 0].min()) >= 0 and float(big.factors[..., 0].max()) <= 2.5 and float(big.factors[..., 1].min()) >= 0.9


def test_the_pca_shift_is_the_loaders_statements():
    p = draw(batch=2, seed=(1, 5))
    gen = torch.Generator().manual_seed(5)
    eigval = torch.Tensor([0.2175, 0.0188, 0.0045])
    eigvec = torch.Tensor([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]])
    for b in range(2):
        for v in range(2):
            alpha = torch.empty(3).normal_(0, 0.1, generator=gen)
            rgb = eigvec.clone().mul(alpha.view(1, 3).expand(3, 3)).mul(eigval.view(1, 3).expand(3, 3)).sum(1).squeeze()     # KITTI.py:33-36
            assert torch.equal(p.pca[b, v], rgb)


def test_a_strength_of_zero_omits_its_operation():
    p = draw(hue=0)                                                          # KITTI12.py's ColorJitter(0.4, 0.4, 0.4, 0)
    assert (p.order[..., 3] == -1).all() and (p.order[..., :3].sort(-1).values == torch.arange(3, dtype=torch.int32)).all()
    assert (p.hue_shift == 0).all()
    p = draw(brightness=0, saturation=0)
    assert (p.order[..., 2:] == -1).all() and (p.order[..., :2].sort(-1).values == torch.tensor([1, 3], dtype=torch.int32)).all()
    assert (p.factors[..., 0] == 1).all() and (p.factors[..., 2] == 1).all()
    p = draw(brightness=0, contrast=0, saturation=0, hue=0, alphastd=0)
    assert (p.order == -1).all() and (p.pca == 0).all() and (p.factors == 1).all()


def test_hue_shift_is_the_uint8_wrap():
    for h in (-0.4, -0.2, -1 / 255, -0.001, 0.0, 0.001, 0.3, 0.4, 0.5, -0.5):
        with np.errstate(over="ignore", invalid="ignore"):
            want = int(np.array(int(h * 255)).astype(np.uint8))              # np.uint8 of a negative float is undefined; of its trunc, a wrap
        assert R.hue_shift_of(h) == want == int(h * 255) % 256, h


def test_the_two_statements_of_the_loader_agree():
    """The numpy statement behind the jitter and the torch one that the decodes' tests compare against (tests/frame_fixtures.py),
    once, bit for bit: all 256 bytes in every channel, both clamps binding, and no shift at all against the statement without one."""
    from frame_fixtures import MEAN, STD, loader_statements
    u8 = torch.stack([torch.arange(256), torch.arange(255, -1, -1), (torch.arange(256) * 7) % 256], -1).to(torch.uint8).reshape(16, 16, 3)
    for pca in ((0.9, -0.9, 0.02), (0.0, 0.0, 0.0)):
        image, view = loader_statements(u8, torch.tensor(pca))
        rimage, rview = R.finish(u8.numpy(), pca, MEAN, STD)
        assert np.array_equal(image.numpy(), rimage) and np.array_equal(view.numpy(), rview)
    assert float(image.min()) >= 0 and float(loader_statements(u8, torch.tensor((0.9, -0.9, 0.02)))[0].max()) == 1.0
    plain = loader_statements(u8)
    assert torch.equal(plain[0], image) and torch.equal(plain[1], view)          # a zero shift and a clamp that never binds: Flying3d's


def test_python_refusals():
    ops = ecm().ops
    rng, gen = random.Random(0), torch.Generator()
    for kw in (dict(brightness=-0.1), dict(hue=0.6), dict(hue=-0.1), dict(contrast=float("nan")), dict(alphastd=float("inf")), dict(saturation="1")):
        with pytest.raises(ValueError):
            ops.jitter_params(2, rng, gen, **kw)
    for batch in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            ops.jitter_params(batch, rng, gen)
    with pytest.raises(ValueError):
        ops.jitter_params(2, np.random, gen)
    u8 = torch.zeros(2, 4, 5, 3, dtype=torch.uint8)
    ok = ([[1, 1, 1]] * 2, [[0, 1, -1, -1]] * 2, [0, 255])
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.color_jitter(u8, *ok)                                            # no CPU fallback
    with pytest.raises(ValueError):
        ops.color_jitter(u8.numpy(), *ok)
    p = draw(batch=2)
    frames = (torch.zeros(2, 8, 9, 6, dtype=torch.uint8), torch.zeros(2, 8, 9))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.frame_prep_jitter(frames, [0, 0], [0, 0], 4, 4, p)
    with pytest.raises(ValueError):
        ops.frame_prep_jitter(torch.zeros(2, 8, 9, 7), [0, 0], [0, 0], 4, 4, p)      # the float32 frame path is not taken
    with pytest.raises(ValueError):
        ops.frame_prep_jitter(frames, [0, 0], [0, 0], 4, 4, None)
    # the parameter checks come before any device work: they are the same function on any device
    views = ops._jitter_views
    assert len(views("t", 2, *ok)) == 3 and len(views("t", 2, *ok, [[0, 0, 0]] * 2)) == 4
    bad = [
        ([[1, 1, 1]], ok[1], ok[2]), ([[1, 1]] * 2, ok[1], ok[2]), ([[1, -0.5, 1]] * 2, ok[1], ok[2]), ([[1, float("nan"), 1]] * 2, ok[1], ok[2]),
        (ok[0], [[0, 0, -1, -1]] * 2, ok[2]), (ok[0], [[0, -1, 1, -1]] * 2, ok[2]), (ok[0], [[4, -1, -1, -1]] * 2, ok[2]),
        (ok[0], [[0, 1, 2]] * 2, ok[2]), (ok[0], [[0.0, 1.0, -1.0, -1.0]] * 2, ok[2]), (ok[0], [[-2, -1, -1, -1]] * 2, ok[2]),
        (ok[0], ok[1], [0, 256]), (ok[0], ok[1], [-1, 0]), (ok[0], ok[1], [0]),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            views("t", 2, *args)
    with pytest.raises(ValueError):
        views("t", 2, *ok, [[0, float("inf"), 0]] * 2)
    S = sys.modules[ops.__name__.rsplit(".", 1)[0] + ".shards"] if ops.__name__.rsplit(".", 1)[0] + ".shards" in sys.modules else \
        __import__("importlib").import_module(ops.__name__.rsplit(".", 1)[0] + ".shards")
    feeder = lambda **kw: S.ShardFeeder(None, 1, **kw)                       # noqa: E731  refused before the reader or a device is touched
    for kw in (dict(jitter=dict(brightness=0.4)), dict(jitter=0.4), dict(jitter=dict(ops.KITTI_JITTER, hue=0.7)),
               dict(jitter=dict(ops.KITTI_JITTER), split="test")):
        with pytest.raises(ValueError):
            feeder(**kw)


# ---- the census of the ninth header -------------------------------------------------------------------------------------------------------
def header_prototypes():
    with open(os.path.join(INCLUDE, HEADER)) as f:
        return parse_header(f.read())


def test_the_registries():
    lib = ecm()._lib
    assert lib.REGISTRIES == (lib.TABLES, lib.EXTENSION_TABLES, lib.MOTION_TABLES) and lib.LATER_REGISTRIES == (lib.VOLUME_TABLES,)
    assert lib.NEWER_REGISTRIES == (lib.MESH_TABLES,) and lib.NEWEST_REGISTRIES == (lib.COLOR_TABLES,) and tuple(lib.COLOR_TABLES) == ("ecm_color.h",)
    before = dict(lib._each_table())
    assert len(before) == sum(len(t) for reg in lib.REGISTRIES + lib.LATER_REGISTRIES + lib.NEWER_REGISTRIES + lib.NEWEST_REGISTRIES
                              for t, _ in reg.values())
    assert not any(n in before for n in ENTRIES)
    assert lib.LATEST_REGISTRIES == (lib.AUGMENT_TABLES,) and tuple(lib.AUGMENT_TABLES) == (HEADER,)
    assert lib.AUGMENT_TABLES[HEADER][0] is lib.AUGMENT_PROTOTYPES and lib.AUGMENT_TABLES[HEADER][1] == PREFIX
    whole = dict(lib._whole_table())
    assert len(whole) == len(before) + len(ENTRIES) and all(n in whole for n in ENTRIES) and all(whole[n] == before[n] for n in before)
    # the earlier walkers keep their results
    assert len(lib._tables()) == sum(len(t) for reg in lib.REGISTRIES for t, _ in reg.values())
    assert len(lib._all_tables()) == len(lib._tables()) + len(lib.VOLUME_PROTOTYPES)
    assert len(lib._every_table()) == len(lib._all_tables()) + len(lib.MESH_PROTOTYPES)
    assert len(lib._each_table()) == len(lib._every_table()) + len(lib.COLOR_PROTOTYPES)


def test_header_table_and_package_literals_name_the_same_entries():
    lib = ecm()._lib
    parsed = header_prototypes()
    with open(os.path.join(INCLUDE, HEADER)) as f:
        by_text = set(re.findall(rf"\b({PREFIX}[a-z0-9_]+)\s*\(", _strip(f.read())))
    found = package_entry_names(PREFIX + "[a-z0-9_]+", "AUGMENT_PROTOTYPES")
    assert sorted(parsed) == sorted(by_text) == sorted(lib.AUGMENT_PROTOTYPES) == sorted(found) == sorted(ENTRIES)
    assert all(n.startswith(PREFIX) for n in parsed)
    assert all(a.startswith("ops.py:") for at in found.values() for a in at), found
    for registry in lib.REGISTRIES + lib.LATER_REGISTRIES + lib.NEWER_REGISTRIES + lib.NEWEST_REGISTRIES:
        for table, _ in registry.values():
            assert not set(table) & set(lib.AUGMENT_PROTOTYPES)


def test_prototypes_match_the_header_type_by_type():
    table, parsed = ecm()._lib.AUGMENT_PROTOTYPES, header_prototypes()
    assert compare(parsed, table) == []
    assert all(table[n] == parsed[n] for n in parsed)


def test_library_exports_every_row_and_load_types_it(lib_mod):
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(lib, n)] == [] and lib_mod.missing_symbols() == []
    table = lib_mod.AUGMENT_PROTOTYPES
    real = dict(table)
    try:
        table[PREFIX + "not_there"] = (C.c_int, [])
        assert lib_mod.missing_symbols() == [PREFIX + "not_there"]
    finally:
        table.clear()
        table.update(real)
    loaded = lib_mod.load()
    for name, (res, args) in table.items():
        assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == args, name
    assert lib_mod.query("ecma_jitter_tile") == TILE == ecm().ops.jitter_tile()
    q = lambda *a: lib_mod.query("ecma_jitter_scratch_bytes", *a)            # noqa: E731
    assert q(1, 37, 53) == 4 and q(24, 70, 131) == 24 * 5 * 4 and q(8, 256, 512) == 8 * 64 * 4 and q(1, 4096, 4096) == 8192 * 4
    assert q(1, 1, TILE) == 4 and q(1, 1, TILE + 1) == 8 and q(3, 65535, 256) == 3 * 8192 * 4
    assert q(1, 4096, 4097) == 0 and q(1, 65536, 1) == 0 and q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, -1) == 0


# ---- the refusal contract, with the devices hidden --------------------------------------------------------------------------------------
_VIEW = "factors:hf{f}@1 order:hi{o}@-1 hue_shift:hi{h}"
ROWS = [
    Row("ecma_color_jitter_fwd", "images:p out:p N=1 H=2 W=2 " + _VIEW.format(f=3, o=4, h=1) + " scratch:p scratch_bytes=Q0 stream:s",
        queries=[("ecma_jitter_scratch_bytes", "N H W")],
        legal=[{"scratch_bytes": 1}],              # the largest legal sizes: test_library_exports_every_row_and_load_types_it, by the query
        # "ECM_EUNSUP: H > 65535 or H * W > 2^24"
        unsup=[{"H": 65536, "W": 1}, {"H": 4096, "W": 4097}, {"H": 65535, "W": 257}], header=HEADER),
    Row("ecma_frame_prep_jitter_fwd",
        "rgb6:p disp_in:p disp_is_half=~0 left:p right:p disp:p image:o B=1 H=8 W=8 crop_y0:hi1 crop_x0:hi1 th=2 tw=2 "
        + _VIEW.format(f=6, o=8, h=2) + " pca:hf6 mean3:hf3 std3:hf3@1 scratch:p scratch_bytes=Q0 stream:s",
        queries=[("ecma_jitter_scratch_bytes", "2*B th tw")],
        legal=[{"disp_is_half": 1}, {"scratch_bytes": 1}],
        # "a window outside its frame": the size query is not given the frame, so it answers for these all the same
        inval=[{"th": 9}, {"tw": 9}, {"H": 1}, {"W": 1}], blind=("th=9", "tw=9"),
        # "ECM_EUNSUP: th > 65535 or th * tw > 2^24"
        unsup=[{"H": 65536, "th": 65536}, {"H": 4096, "W": 4097, "th": 4096, "tw": 4097}], header=HEADER),
]
QUERIES = [Row("ecma_jitter_scratch_bytes", "views=1 rows=2 cols=2", header=HEADER)]
INT_CONSTS = ("ecma_jitter_tile",)


@pytest.fixture(scope="module")
def results(lib_mod):
    """{call id: return value} of the rows above from one fresh child that sees no device (tests/abi_refusal_child.py)."""
    parsed = header_prototypes()
    calls = [{"id": f"const|{n}", "fn": n, "res": "i", "args": []} for n in INT_CONSTS]
    for row in ROWS:
        calls += calls_of(row, lambda q: parsed[q][1])
    for row in QUERIES:
        calls += query_calls(row)
    assert len({c["id"] for c in calls}) == len(calls)
    env = dict(os.environ)
    env.update(HIDE)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__)], input=json.dumps({"lib": lib_mod.LIB_PATH, "calls": calls}),
                       capture_output=True, text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    seen = next((ln.split()[1] for ln in lines if ln.startswith("DEVICES ")), None)
    assert seen is not None and seen.isdigit(), f"the child did not report a device count (exit {r.returncode}): {r.stderr[-2000:]}"
    if seen != "0":
        pytest.skip(f"the child sees {seen} device(s) although {sorted(HIDE)} hide them: no ABI call was made")
    got = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("R ")}
    if "DONE" not in lines:
        nxt = next((c["id"] for c in calls if c["id"] not in got), None)
        pytest.fail(f"the child ended with status {r.returncode} in call {nxt}: {r.stderr[-2000:]}")
    return got


def test_every_entry_of_the_ninth_header_has_a_row():
    parsed = header_prototypes()
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    assert sorted(ent) == sorted(r.name for r in ROWS) and sorted(qry) == sorted(r.name for r in QUERIES)
    for r in ROWS + QUERIES:
        assert r.types == parsed[r.name][1], r.name
    assert sorted(set(parsed) - set(ent) - set(qry)) == list(INT_CONSTS)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    row = next(r for r in ROWS if r.name == name)
    bad = classify(row, results)
    assert not bad, "\n" + _report(bad)
    assert results[f"{name}|accepted"] > 0                                 # the pointers are never dereferenced: no device, no crash
    assert results[f"{name}|scratch_bytes=query-1"] == ESCRATCH            # one byte short
    assert results["const|ecma_jitter_tile"] == TILE


def test_the_size_query_is_zero_for_sizes_it_cannot_serve(results):
    bad = classify_query(QUERIES[0], results)
    assert not bad, "\n" + _report(bad)


def test_further_refusals_of_the_entries(lib_mod):
    """What the rows cannot express: the contents of the host arrays, and an output that is the input.  Every call returns before
    any HIP call."""
    lib = lib_mod.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(8)]                     # never dereferenced
    host = lambda t, v: C.cast((t * len(v))(*v), C.c_void_p)               # noqa: E731
    orders = {"ok": [0, 1, -1, -1], "twice": [0, 0, -1, -1], "gap": [0, -1, 1, -1], "code 4": [4, -1, -1, -1], "code -2": [-2, -1, -1, -1]}

    def jitter(order="ok", shift=0, out=p[1], nbytes=4):
        return lib.ecma_color_jitter_fwd(p[0], out, 1, 2, 2, host(C.c_float, [1, 1, 1]), host(C.c_int, orders[order]), host(C.c_int, [shift]),
                                         p[2], C.c_longlong(nbytes), None)
    for order in list(orders)[1:]:
        assert jitter(order) == EINVAL, order
    assert jitter(shift=-1) == EINVAL and jitter(shift=256) == EINVAL and jitter(out=p[0]) == EINVAL
    assert jitter(nbytes=3) == ESCRATCH and jitter(nbytes=0) == ESCRATCH

    def prep(order=orders["ok"] * 2, shift=(0, 0), ys=(6,), xs=(6,), nbytes=8):
        return lib.ecma_frame_prep_jitter_fwd(p[0], p[1], 0, p[2], p[3], p[4], None, 1, 8, 8, host(C.c_int, ys), host(C.c_int, xs), 2, 2,
                                              host(C.c_float, [1] * 6), host(C.c_int, order), host(C.c_int, shift), host(C.c_float, [0] * 6),
                                              host(C.c_float, [0] * 3), host(C.c_float, [1] * 3), p[5], C.c_longlong(nbytes), None)
    for name in list(orders)[1:]:
        assert prep(order=orders["ok"] + orders[name]) == EINVAL, name       # the right view's order is checked too
    assert prep(shift=(0, 256)) == EINVAL and prep(shift=(-1, 0)) == EINVAL
    for kw in (dict(ys=(7,)), dict(xs=(7,)), dict(ys=(-1,)), dict(xs=(-1,))):
        assert prep(**kw) == EINVAL, kw
    assert prep(nbytes=7) == ESCRATCH
    # no legal call is made here: this process may see a device, and the pointers are not device memory
