"""mesh.volume_mesh and models.StereoMapper.mesh on the MI355X against mesh_t of
tests/test_volume_mesh_cpu.py, run on the CPU.

The counts and the faces must be equal.  The per-vertex arithmetic of the device is the restatement's, operation for operation
(IEEE fp64 without fused multiply-adds, rounded once to fp32), so bit-equality is expected of vertices, normals and weights; one
ulp of fp32 is allowed, and every comparison prints whether the three were bit-equal.  Volumes: one cube (2x2x2), the random
volume in which every (tetrahedron, case) pair occurs, one classification brick exactly and a brick plus one point on each
axis, thin volumes along x and along z, more points than one tile of the compaction and than two, a volume with unweighted
holes, empty meshes, and the three-plane scene integrated on the device.  There is no vector-load path: the planes are read
four bytes at a time, which the misaligned variant runs all the same.  Then the forward-only operand contract of DESIGN.md section 34, with
the builders of tests/forward_contract_table.py: misaligned planes, a side stream, a second call, recycled NaN memory, guard
bands around the four outputs, the counts and the scratch, inputs untouched, and capacities one row short."""
import ctypes as C

import pytest
import torch

import forward_contract_table as FT
from test_disp_warp_cpu import rigid
from test_hip_guard_bands import guarded
from test_volume_mesh_cpu import ALL_CASES_DIMS, BRICK, F32, F64, TILE, all_cases, mesh_t, random_volume, sphere_volume, unmatched_edges

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORIGIN, VOXEL = (-0.4, 0.3, 1.25), 0.0625
POSE = rigid(0.02, -0.03, 0.01, 0.1, -0.2, 0.05)


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def ulps(a, b):
    return FT._ulps(a, b)


def held(ecm, tsdf, wsum, label, T=None, min_weight=0.0, want=None):
    """mesh.volume_mesh of the volume on the device against mesh_t; (the device's Mesh on the CPU, the restatement)."""
    mesh = ecm.mesh
    M = mesh.mesh_matrix(ORIGIN, VOXEL, T)
    want = mesh_t(tsdf, wsum, M, min_weight) if want is None else want
    got = mesh.volume_mesh(tsdf.to(DEV), wsum.to(DEV), ORIGIN, VOXEL, T, min_weight, with_normals=True, with_weight=True)
    assert isinstance(got, mesh.Mesh) and all(t.device.type == "cuda" for t in got)
    got = mesh.Mesh(*(t.cpu() for t in got))
    N, F = len(want.vertices), len(want.faces)
    assert got.vertices.shape == (N, 3) and got.faces.shape == (F, 3) and got.normals.shape == (N, 3) and got.weight.shape == (N,), \
        (label, tuple(got.vertices.shape), tuple(got.faces.shape), N, F)
    assert got.vertices.dtype == F32 and got.faces.dtype == torch.int32 and got.normals.dtype == F32 and got.weight.dtype == F32
    assert torch.equal(got.faces, want.faces), label
    seen = (ulps(got.vertices, want.vertices), ulps(got.normals, want.normals), ulps(got.weight, want.weight))
    equal = tuple(FT.bits_equal(a, b) for a, b in ((got.vertices, want.vertices), (got.normals, want.normals), (got.weight, want.weight)))
    print("mesh", label, "N", N, "F", F, "ulps (vertices, normals, weight)", seen, "bit-equal", equal)
    assert max(seen) <= 1, (label, seen)
    return got, want


def dims_of():
    bx, by, bz = BRICK
    return {"one cube": (2, 2, 2), "one brick": (bz, by, bx), "a brick plus one": (bz + 1, by + 1, bx + 1), "thin along x": (2, 5, 70),
            "thin along z": (70, 5, 2), "two bricks along y and z": (2 * bz, 2 * by, 3), "more than one tile": (9, 17, 33),
            "two tiles and eight points": (3, 3, (2 * TILE + 8) // 9)}      # 3 * 3 * 456 = 2 * 2048 + 8


@pytest.mark.parametrize("name", list(dims_of()))
def test_random_volumes_against_the_restatement(ecm, name):
    dims = dims_of()[name]
    tsdf, wsum = random_volume(dims, sum(dims))
    got, want = held(ecm, tsdf, wsum, f"{name} {dims}", T=POSE if name != "one cube" else None)
    assert len(want.faces) > 0 and int(got.faces.max()) < len(got.vertices) and len(torch.unique(got.faces)) == len(got.vertices)
    ecm.ops.check_async_errors()


def test_every_case_and_the_world_frame(ecm):
    tsdf, wsum, _ = all_cases()
    assert tuple(tsdf.shape) == ALL_CASES_DIMS
    got, want = held(ecm, tsdf, wsum, "all 96 cases")
    assert len(want.cases) == 96
    cam, _ = held(ecm, tsdf, wsum, "all 96 cases, a camera's frame", T=POSE)
    assert torch.equal(cam.faces, got.faces) and not torch.equal(cam.vertices, got.vertices)
    # the option flags leave out what they say and nothing else
    bare = ecm.mesh.volume_mesh(tsdf.to(DEV), wsum.to(DEV), ORIGIN, VOXEL, with_normals=False)
    assert bare.normals is None and bare.weight is None and FT.bits_equal(bare.vertices.cpu(), got.vertices) and torch.equal(bare.faces.cpu(), got.faces)


def test_holes_zeros_and_min_weight(ecm):
    dims = (9, 10, 21)
    tsdf, wsum = random_volume(dims, 5, holes=0.05)
    tsdf[torch.rand(dims, generator=torch.Generator().manual_seed(6)) < 0.05] = 0.0              # exact zeros: a = 0 or 1
    tsdf[torch.rand(dims, generator=torch.Generator().manual_seed(7)) < 0.02] = -0.0
    tsdf[2, 3, 4], tsdf[5, 5, 5], wsum[1, 1, 1] = float("nan"), float("inf"), float("nan")
    got, want = held(ecm, tsdf, wsum, "holes, zeros, NaN")
    full = mesh_t(tsdf, torch.ones(dims), ecm.mesh.mesh_matrix(ORIGIN, VOXEL))
    assert 0 < len(want.faces) < len(full.faces) and len(unmatched_edges(want)) > 0
    assert bool(torch.isfinite(got.vertices).all()) and bool(torch.isfinite(got.normals).all())
    gated, _ = held(ecm, tsdf, wsum, "min_weight 1.5", min_weight=1.5)
    assert 0 < len(gated.faces) < len(got.faces)


def test_empty_meshes(ecm):
    for label, tsdf, wsum in (("all positive", torch.ones(5, 6, 7), torch.ones(5, 6, 7)), ("all negative", -torch.ones(5, 6, 7), torch.ones(5, 6, 7)),
                              ("no weight", random_volume((5, 6, 7), 1)[0], torch.zeros(5, 6, 7)),
                              ("a new volume", torch.ones(2, 2, 2), torch.zeros(2, 2, 2))):
        got, _ = held(ecm, tsdf, wsum, label)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals.shape == (0, 3) and got.weight.shape == (0,)
    ecm.ops.check_async_errors()


def test_a_sphere_is_closed_on_the_device(ecm):
    tsdf, wsum = sphere_volume(20, 6.1)
    got, want = held(ecm, tsdf, wsum, "sphere")
    assert len(unmatched_edges(want)) == 0
    c = ecm.mesh.mesh_matrix(ORIGIN, VOXEL)[:3] @ torch.tensor([9.5, 9.5, 9.5, 1.0], dtype=F64)
    assert bool(((got.normals.to(F64) * (got.vertices.to(F64) - c)).sum(1) > 0).all())


def test_the_three_plane_scene_integrated_on_the_device(ecm):
    from test_disp_volume_cpu import DIMS, TRUNC, VIEWS, scene_views
    from test_disp_volume_cpu import ORIGIN as O, VOXEL as V
    ops, mesh = ecm.ops, ecm.mesh
    disp, Q = scene_views()
    vol = ops.volume_new(DIMS, DEV)
    ops.volume_integrate(*vol, disp.to(DEV), Q, torch.stack(VIEWS), O, V, TRUNC)
    tsdf, wsum = vol[0].cpu(), vol[1].cpu()
    want = mesh_t(tsdf, wsum, mesh.mesh_matrix(O, V))
    got = mesh.Mesh(*(t.cpu() for t in mesh.volume_mesh(*vol, O, V, with_weight=True)))
    seen = (ulps(got.vertices, want.vertices), ulps(got.normals, want.normals), ulps(got.weight, want.weight))
    print("three-plane scene: N", len(want.vertices), "F", len(want.faces), "ulps", seen)
    assert torch.equal(got.faces, want.faces) and len(want.faces) > 1000 and max(seen) <= 1
    # the surface lies at about 3 m in front of the first camera, and its normals look back at it
    z = got.vertices[:, 2]
    assert 2.0 < float(z.min()) and float(z.max()) < 4.6 and bool((got.normals[:, 2] < 0).all())


# ---- the forward-only operand contract ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean(ecm):
    """The contract's volume (a brick plus one, with holes), its planes on the device and the clean result."""
    bx, by, bz = BRICK
    tsdf, wsum = random_volume((bz + 1, by + 1, bx + 1), 17, holes=0.03)
    got, want = held(ecm, tsdf, wsum, "contract volume", T=POSE)
    assert len(want.faces) > 100
    return tsdf.to(DEV), wsum.to(DEV), got


def run(ecm, tsdf, wsum):
    return ecm.mesh.volume_mesh(tsdf, wsum, ORIGIN, VOXEL, POSE, with_normals=True, with_weight=True)


def same(got, want, what):
    for name, g, w in zip(("vertices", "faces", "normals", "weight"), got, want):
        assert FT.bits_equal(g.cpu(), w), f"{what}: {name}"


def test_misaligned_planes(ecm, clean):
    tsdf, wsum, want = clean
    for label, t, w in (("tsdf", FT.misaligned(tsdf), wsum), ("wsum", tsdf, FT.misaligned(wsum)), ("both", FT.misaligned(tsdf), FT.misaligned(wsum))):
        assert (t.data_ptr() % 16 == 4) == (label != "wsum") and (w.data_ptr() % 16 == 4) == (label != "tsdf")
        same(run(ecm, t, w), want, f"{label} 4 bytes off a 16-byte boundary")
    ecm.ops.check_async_errors()


def test_side_stream_and_a_second_call(ecm, clean):
    tsdf, wsum, want = clean
    x = torch.randn(2048, 2048, device=DEV)
    out = torch.empty_like(x)
    t, w = torch.full_like(tsdf, float("nan")), torch.full_like(wsum, float("nan"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.matmul(x, x, out=out)                                        # the planes are written behind this, on the side stream
        t.copy_(tsdf, non_blocking=True)
        w.copy_(wsum, non_blocking=True)
        got = run(ecm, t, w)
        s.synchronize()
    same(got, want, "on a side stream")
    same(run(ecm, tsdf, wsum), want, "a second call")
    ecm.ops.check_async_errors()


def test_recycled_memory_guard_bands_and_untouched_inputs(ecm, clean):
    tsdf, wsum, want = clean
    before = (tsdf.clone(), wsum.clone())
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 6, 1 << 10, 1 << 14, 1 << 17, 1 << 19) for _ in range(4)]
    torch.cuda.synchronize()
    del junk                                                               # the allocator's free blocks now hold NaN ...
    same(run(ecm, tsdf, wsum), want, "on recycled memory")               # ... and outputs and scratch come from them
    with guarded(ecm) as g:
        got = run(ecm, tsdf, wsum)
        g.check("volume_mesh")
        assert len(g.records) == 6                                         # scratch, counts, vertices, faces, normals, weight
    same(got, want, "between guard bands")
    assert FT.bits_equal(tsdf, before[0]) and FT.bits_equal(wsum, before[1])
    ecm.ops.check_async_errors()


def test_a_capacity_one_row_short(ecm, clean):
    """The C entries themselves: the rows that fit are written and the row beyond the capacity keeps its bits."""
    tsdf, wsum, want = clean
    lib, ops, mesh = ecm._lib, ecm.ops, ecm.mesh
    nz, ny, nx = tsdf.shape
    need = lib.query("ecms_mesh_scratch_bytes", nx, ny, nz)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    lib.call("ecms_mesh_count_fwd", ops._p(tsdf), ops._p(wsum), ops._p(counts), ops._p(scratch), C.c_longlong(need), nx, ny, nz, 0.0, ops._stream())
    N, F = counts.tolist()
    assert (N, F) == (len(want.vertices), len(want.faces))
    M = mesh.mesh_matrix(ORIGIN, VOXEL, POSE).to(DEV)
    mark = 12345.0
    vertices, normals = torch.full((N, 3), mark, device=DEV), torch.full((N, 3), mark, device=DEV)
    weight, faces = torch.full((N,), mark, device=DEV), torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
    lib.call("ecms_mesh_emit_fwd", ops._p(tsdf), ops._p(wsum), ops._p(M), ops._p(vertices), ops._p(faces), ops._p(normals), ops._p(weight),
             ops._p(scratch), C.c_longlong(need), C.c_longlong(N - 1), C.c_longlong(F - 1), nx, ny, nz, 0.0, ops._stream())
    torch.cuda.synchronize()
    for name, got, full in (("vertices", vertices, want.vertices), ("normals", normals, want.normals), ("weight", weight, want.weight),
                            ("faces", faces, want.faces)):
        got = got.cpu()
        assert FT.bits_equal(got[:-1], full[:-1]), name
        assert bool((got[-1] == (-7 if name == "faces" else mark)).all()), name
    ops.check_async_errors()


def test_stereo_mapper_mesh_after_two_frames(ecm):
    from test_disp_volume_cpu import DIMS, H0, MAPPER_MIN_DISP, MAPPER_STD, TRUNC, W0, mapper_maps
    from test_disp_volume_cpu import ORIGIN as O, VOXEL as V
    from test_hip_motion_align import Stub
    models = ecm.models
    maps, Q = mapper_maps()
    mapper = models.StereoMapper(ecm.get_model("cmfsm"), Q, O, V, DIMS, TRUNC, min_disp=MAPPER_MIN_DISP, step=1)
    mapper.odometry.tracker.model = Stub([m[None, None].to(DEV) for m in maps[:2]], MAPPER_STD)
    x = torch.zeros(1, 3, H0, W0, device=DEV)
    for _ in range(2):
        assert mapper(x, x).integrated
    m = mapper.mesh()
    assert isinstance(m, ecm.mesh.Mesh) and m.weight is None and m.normals is not None
    N, F = len(m.vertices), len(m.faces)
    print("StereoMapper.mesh after two frames: N", N, "F", F)
    assert N > 0 and F > 0 and bool(torch.isfinite(m.vertices).all()) and bool(torch.isfinite(m.normals).all())
    assert int(m.faces.min()) >= 0 and int(m.faces.max()) < N
    want = mesh_t(mapper.volume[0].cpu(), mapper.volume[1].cpu(), ecm.mesh.mesh_matrix(O, V))
    assert torch.equal(m.faces.cpu(), want.faces) and ulps(m.vertices.cpu(), want.vertices) <= 1
    none = mapper.mesh(min_weight=64.0, with_weight=True)                  # wsum is clamped to max_weight = 64: nothing lies above it
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3) and none.weight.shape == (0,)
    ecm.ops.check_async_errors()
