"""The mesh of the TSDF volume without a GPU: mesh_t, an fp64 numpy restatement of include/ecm_mesh.h
written from the header's text, which builds the triangle table from the header's rule; the table of csrc/disp_mesh.hip against
it; the surface's topology edge by edge on a random volume in which every (tetrahedron, case) pair occurs; a sphere; every
decision on hand-made volumes; mesh.volume_mesh's matrices and refusals; mesh.write_ply; the seventh header's census and refusal
contract.  tests/test_hip_volume_mesh.py compares the device with mesh_t.

Every operation of the restatement is one numpy operation in the header's order (separate elementwise calls: nothing is fused),
so every value is the header's bit for bit."""
import collections
import ctypes as C
import inspect
import itertools
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_refusal_child as child
from test_abi_refusals import EINVAL, EUNSUP, HIDE, Row, _report, calls_of, classify
from test_abi_types import INCLUDE, PACKAGE, _strip, compare, lib_mod, package_entry_names, parse_header  # noqa: F401  (lib_mod: a fixture)
from test_disp_warp_cpu import rigid
from test_motion_align_cpu import fake

HEADER = "ecm_mesh.h"
PREFIX = "ecms_"
ENTRIES = ("ecms_mesh_brick", "ecms_mesh_count_fwd", "ecms_mesh_emit_fwd", "ecms_mesh_scratch_bytes", "ecms_mesh_tile")
NAN, INF = float("nan"), float("inf")
F64, F32 = torch.float64, torch.float32
TILE, BRICK = 2048, (16, 4, 4)
MAX_POINTS = 1 << 27


def ecm():
    import ecm_amd
    return ecm_amd


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))                           # lexicographic


def tet_corners(tet):
    """The four corners of tetrahedron `tet` of the unit cube, as (x, y, z) tuples."""
    a0, a1, _ = PERMS[tet]
    c1 = [0, 0, 0]
    c1[a0] = 1
    c2 = list(c1)
    c2[a1] = 1
    return (0, 0, 0), tuple(c1), tuple(c2), (1, 1, 1)


def _slot(lo, hi):
    """The edge between two corners lo <= hi of the cube as (offset of its starting point, dir)."""
    return lo, DIRS.index(tuple(h - l for l, h in zip(lo, hi)))


def build_table():
    """table[tet][case] = the triangles of the case, each three slots ((ox, oy, oz), dir) relative to the cube: the header's rule."""
    table = []
    for tet in range(6):
        c = [np.array(p, dtype=np.float64) for p in tet_corners(tet)]
        rows = []
        for case in range(16):
            pos = [k for k in range(4) if case >> k & 1]
            neg = [k for k in range(4) if not case >> k & 1]
            edge = lambda a, b: (min(a, b), max(a, b))                                           # noqa: E731
            if len(pos) in (1, 3):
                lone = pos[0] if len(pos) == 1 else neg[0]
                tris = [[edge(lone, k) for k in range(4) if k != lone]]
            elif len(pos) == 2:
                q = [edge(pos[0], neg[0]), edge(pos[0], neg[1]), edge(pos[1], neg[1]), edge(pos[1], neg[0])]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                tris = []
            out = []
            for tri in tris:
                v = [(c[a] + c[b]) / 2 for a, b in tri]
                side = sum(c[k] for k in pos) / len(pos) - sum(c[k] for k in neg) / len(neg)
                s = float(np.dot(np.cross(v[1] - v[0], v[2] - v[0]), side))
                assert s != 0.0
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                out.append(tuple(_slot(tuple(int(x) for x in c[a]), tuple(int(x) for x in c[b])) for a, b in tri))
            rows.append(tuple(out))
        table.append(tuple(rows))
    return tuple(table)


TABLE = build_table()
Restated = collections.namedtuple("Restated", "vertices faces normals weight slots cases")


def _shift(a, d, fill):
    """a[z + dz, y + dy, x + dx] with `fill` outside the grid, d = (dx, dy, dz) in {-1, 0, 1}."""
    out = np.full_like(a, fill)
    nz, ny, nx = a.shape
    src = tuple(slice(max(s, 0), n + min(s, 0)) for s, n in zip(d[::-1], (nz, ny, nx)))
    dst = tuple(slice(max(-s, 0), n + min(-s, 0)) for s, n in zip(d[::-1], (nz, ny, nx)))
    out[dst] = a[src]
    return out


def _gradient(t, usable):
    """The header's gradient at every grid point: [3, nz, ny, nx] fp64."""
    t64 = t.astype(np.float64)
    out = []
    for axis in range(3):
        e = tuple(int(a == axis) for a in range(3))
        m = tuple(-v for v in e)
        hi, lo = _shift(t64, e, 0.0), _shift(t64, m, 0.0)
        has_hi, has_lo = _shift(usable, e, False), _shift(usable, m, False)
        both, fwd, bwd = hi - lo, hi - t64, t64 - lo
        out.append(np.where(has_hi & has_lo, both, np.where(has_hi, fwd, np.where(has_lo, bwd, 0.0))))
    return np.stack(out)


def mesh_t(tsdf, wsum, M, min_weight=0.0):
    """include/ecm_mesh.h on CPU tensors: Restated(vertices [N,3] fp32, faces [F,3] int32, normals [N,3] fp32, weight [N] fp32,
    slots [N,4] (x, y, z, dir) and cases, the set of (tetrahedron, case) pairs of the live cubes), torch tensors but for the set."""
    with np.errstate(all="ignore"):
        return _mesh_t(tsdf, wsum, M, min_weight)


def _mesh_t(tsdf, wsum, M, min_weight):
    t, w = tsdf.numpy(), wsum.numpy()
    M = M.numpy()
    nz, ny, nx = t.shape
    usable = (w > np.float32(min_weight)) & np.isfinite(t)
    pos = t > 0
    live = np.zeros_like(usable)                                           # cube (i, j, k) at its low corner; the last planes stay dead
    lv = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        lv &= usable[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    live[:nz - 1, :ny - 1, :nx - 1] = lv
    # the slots
    has = np.zeros((nz, ny, nx, 7), dtype=bool)
    for d, dr in enumerate(DIRS):
        differ = pos != _shift(pos, dr, False)
        within = np.zeros_like(usable)
        for back in itertools.product(*[(0,) if v else (0, 1) for v in dr]):
            within |= _shift(live, tuple(-b for b in back), False)
        has[..., d] = differ & within
    number = (np.cumsum(has.reshape(-1)) - 1).reshape(has.shape)
    kk, jj, ii, dd = np.nonzero(has)                                       # in the order (linear index of p, dir)
    N = len(ii)
    dr = np.array(DIRS)[dd]
    qi, qj, qk = ii + dr[:, 0], jj + dr[:, 1], kk + dr[:, 2]
    t0, t1 = t[kk, jj, ii].astype(np.float64), t[qk, qj, qi].astype(np.float64)
    a = t0 / (t0 - t1)
    g = [ii + dr[:, 0] * a, jj + dr[:, 1] * a, kk + dr[:, 2] * a]
    vertices = np.stack([(((M[r, 0] * g[0] + M[r, 1] * g[1]) + M[r, 2] * g[2]) + M[r, 3]).astype(np.float32) for r in range(3)], 1)
    G = _gradient(t, usable)
    n = [G[ax][kk, jj, ii] + a * (G[ax][qk, qj, qi] - G[ax][kk, jj, ii]) for ax in range(3)]
    m = [(M[r, 0] * n[0] + M[r, 1] * n[1]) + M[r, 2] * n[2] for r in range(3)]
    ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    ok = np.isfinite(ln) & (ln != 0)
    normals = np.stack([np.where(ok, m[r] / ln, 0.0).astype(np.float32) for r in range(3)], 1)
    w0, w1 = w[kk, jj, ii].astype(np.float64), w[qk, qj, qi].astype(np.float64)
    weight = (w0 + a * (w1 - w0)).astype(np.float32)
    # the faces
    ck, cj, ci = np.nonzero(live)                                          # linear order
    rows, cases = [], set()
    for tet in range(6):
        corners = tet_corners(tet)
        case = np.zeros(len(ci), dtype=np.int64)
        for b, (ox, oy, oz) in enumerate(corners):
            case |= pos[ck + oz, cj + oy, ci + ox].astype(np.int64) << b
        for cs in np.unique(case):
            cases.add((tet, int(cs)))
            sel = np.nonzero(case == cs)[0]
            for k, tri in enumerate(TABLE[tet][cs]):
                ids = [number[ck[sel] + o[2], cj[sel] + o[1], ci[sel] + o[0], d] for o, d in tri]
                for (o, d), col in zip(tri, ids):
                    assert bool(has[ck[sel] + o[2], cj[sel] + o[1], ci[sel] + o[0], d].all())     # every referenced slot has a vertex
                rows.append(np.stack([sel, np.full_like(sel, tet), np.full_like(sel, k)] + ids, 1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 6), dtype=np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    faces = rows[:, 3:].astype(np.int32)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))              # noqa: E731
    return Restated(tt(vertices).reshape(N, 3), tt(faces).reshape(-1, 3), tt(normals).reshape(N, 3), tt(weight),
                    tt(np.stack([ii, jj, kk, dd], 1)), cases)


def grid_matrix(origin=(0.0, 0.0, 0.0), voxel=1.0):
    S = torch.eye(4, dtype=F64)
    S[0, 0] = S[1, 1] = S[2, 2] = voxel
    S[:3, 3] = torch.tensor(origin, dtype=F64)
    return S


EYE = torch.eye(4, dtype=F64)


# ---- the volumes the GPU test shares ----------------------------------------------------------------------------------------------------
ALL_CASES_SEED = 0
ALL_CASES_DIMS = (8, 7, 6)                                                 # nz, ny, nx: the issue's "about 6 x 7 x 8"


def random_volume(dims, seed, holes=0.0):
    """tsdf uniform in [-1, 1], wsum in [0.5, 3] with a share `holes` of it zero."""
    g = torch.Generator().manual_seed(seed)
    tsdf = 2 * torch.rand(dims, generator=g) - 1
    wsum = 0.5 + 2.5 * torch.rand(dims, generator=g)
    if holes:
        wsum[torch.rand(dims, generator=g) < holes] = 0.0
    return tsdf.to(F32), wsum.to(F32)


def sphere_volume(n, radius, trunc=2.0):
    """The truncated distance to a sphere about the centre of an n^3 grid, positive outside."""
    c = (n - 1) / 2
    k, j, i = torch.meshgrid(*[torch.arange(n, dtype=F64)] * 3, indexing="ij")
    r = torch.sqrt((i - c) ** 2 + (j - c) ** 2 + (k - c) ** 2)
    return ((r - radius) / trunc).clamp(-1, 1).to(F32), torch.ones(n, n, n)


_ONCE = {}


def all_cases():
    if "all" not in _ONCE:
        tsdf, wsum = random_volume(ALL_CASES_DIMS, ALL_CASES_SEED)
        _ONCE["all"] = (tsdf, wsum, mesh_t(tsdf, wsum, EYE))
    return _ONCE["all"]


# ---- the table --------------------------------------------------------------------------------------------------------------------------
def encode_table(table=TABLE):
    """The table as csrc/disp_mesh.hip packs it: per (tet, case) two words, a triangle as three 6-bit slots (corner x | y << 1 |
    z << 2, dir << 3), an absent triangle all ones."""
    words = []
    for tet in range(6):
        for case in range(16):
            tris = table[tet][case]
            for k in range(2):
                if k < len(tris):
                    words.append(sum(((o[0] | o[1] << 1 | o[2] << 2) | d << 3) << (6 * j) for j, (o, d) in enumerate(tris[k])))
                else:
                    words.append(0xFFFFFFFF)
    return words


def kernel_table():
    with open(os.path.join(PACKAGE, "csrc", "disp_mesh.hip")) as f:
        src = f.read()
    body = re.search(r"TRI_TABLE\[6 \* 16 \* 2\] = \{(.*?)\};", src, flags=re.S).group(1)
    return [int(v, 16) for v in re.findall(r"0x[0-9a-fA-F]+", body)]


def test_the_kernels_table_is_the_rules():
    assert kernel_table() == encode_table() and len(encode_table()) == 192
    counts = [[len(TABLE[t][c]) for c in range(16)] for t in range(6)]
    assert all(row == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0] for row in counts)
    for tet in range(6):                                                   # the six tetrahedra tile the cube: volumes of 1/6, shared chain
        c = np.array(tet_corners(tet), dtype=np.float64)
        assert abs(np.linalg.det(c[1:] - c[0])) == 1.0
    assert len({tet_corners(t) for t in range(6)}) == 6


# ---- topology ---------------------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = faces.numpy().astype(np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def slot_ends(slots):
    """The two grid points of every slot: ([N,3], [N,3])."""
    s = slots.numpy()
    return s[:, :3], s[:, :3] + np.array(DIRS)[s[:, 3]]


def unmatched_edges(res):
    """The directed edges whose reverse is missing, as vertex-number pairs; asserts that no directed edge occurs twice."""
    e = directed_edges(res.faces)
    key = e[:, 0] * (len(res.vertices) + 1) + e[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge is used twice"
    rev = e[:, 1] * (len(res.vertices) + 1) + e[:, 0]
    return e[~np.isin(key, rev)]


def in_one_boundary_face(points, dims):
    """Per row of points [n, k, 3]: all k points lie in one of the six boundary faces of the grid."""
    nz, ny, nx = dims
    out = np.zeros(len(points), dtype=bool)
    for axis, n in enumerate((nx, ny, nz)):
        for side in (0, n - 1):
            out |= (points[:, :, axis] == side).all(1)
    return out


def test_every_case_occurs_and_the_surface_is_closed_off_the_boundary():
    tsdf, wsum, res = all_cases()
    assert len(res.cases) == 96, sorted(set(itertools.product(range(6), range(16))) - res.cases)
    N, F = len(res.vertices), len(res.faces)
    assert N > 0 and F > 0 and int(res.faces.min()) >= 0 and int(res.faces.max()) < N
    assert len(torch.unique(res.faces)) == N                               # every vertex is referenced
    open_ = unmatched_edges(res)
    lo, hi = slot_ends(res.slots)
    ends = np.stack([lo[open_[:, 0]], hi[open_[:, 0]], lo[open_[:, 1]], hi[open_[:, 1]]], 1)
    assert bool(in_one_boundary_face(ends, tsdf.shape).all())
    print("all cases: N", N, "F", F, "directed edges", 3 * F, "without a reverse (all in a boundary face)", len(open_))
    assert len(open_) > 0


def test_holes_open_the_surface_only_beside_dead_cubes():
    dims = (7, 8, 9)
    tsdf, wsum = random_volume(dims, 3, holes=0.04)
    res = mesh_t(tsdf, wsum, EYE)
    full = mesh_t(tsdf, torch.ones(dims), EYE)
    assert 0 < len(res.faces) < len(full.faces)
    assert len(torch.unique(res.faces)) == len(res.vertices) and int(res.faces.max()) < len(res.vertices)
    usable = (wsum > 0).numpy()
    nz, ny, nx = dims
    dead = np.ones((nz + 1, ny + 1, nx + 1), dtype=bool)                    # cube (i, j, k) at [k + 1, j + 1, i + 1]; outside: dead
    lv = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        lv &= usable[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    dead[1:nz, 1:ny, 1:nx] = ~lv
    open_ = unmatched_edges(res)
    lo, hi = slot_ends(res.slots)
    ends = np.stack([lo[open_[:, 0]], hi[open_[:, 0]], lo[open_[:, 1]], hi[open_[:, 1]]], 1)          # [n, 4, 3]
    # an open edge lies in a face of the cubes' lattice (its four end points share one coordinate); one of the two cubes on
    # either side of that face, among those that contain all four points, is dead or outside the grid
    for pts in ends:
        found = False
        for axis in range(3):
            if len(set(pts[:, axis])) != 1:
                continue
            other = [a for a in range(3) if a != axis]
            low = [int(pts[:, a].min()) for a in range(3)]
            if any(int(pts[:, a].max()) - low[a] > 1 for a in other):
                continue
            for side in (-1, 0):
                c = list(low)
                c[axis] += side
                found |= bool(dead[c[2] + 1, c[1] + 1, c[0] + 1])
        assert found, pts
    print("holes: faces", len(res.faces), "of", len(full.faces), "open directed edges", len(open_))


# ---- a sphere ---------------------------------------------------------------------------------------------------------------------------
SPHERE_N, SPHERE_R = 20, 6.1
# The signed volume of the sphere's mesh falls short of 4 pi r^3 / 3 by this share, as test_sphere prints it: the chords of the
# triangles lie inside the sphere and the clamped distance is interpolated linearly.  It comes from the discretisation, not from
# rounding; the bound is twice it.
MEASURED_SPHERE_VOLUME_ERROR = 0.0134
SPHERE_VOLUME_BOUND = 2 * MEASURED_SPHERE_VOLUME_ERROR


def signed_volume(vertices, faces):
    v = vertices.to(F64)[faces.long()]
    return float((v[:, 0] * torch.linalg.cross(v[:, 1], v[:, 2])).sum() / 6)


def sphere():
    if "sphere" not in _ONCE:
        tsdf, wsum = sphere_volume(SPHERE_N, SPHERE_R)
        _ONCE["sphere"] = (tsdf, wsum, mesh_t(tsdf, wsum, EYE))
    return _ONCE["sphere"]


def test_sphere():
    tsdf, wsum, res = sphere()
    V, F = len(res.vertices), len(res.faces)
    e = directed_edges(res.faces)
    E = len(np.unique(np.sort(e, 1), axis=0))
    assert len(unmatched_edges(res)) == 0 and V - E + F == 2, (V, E, F)
    c = (SPHERE_N - 1) / 2
    radial = res.vertices.to(F64) - c
    assert bool(((res.normals.to(F64) * radial).sum(1) > 0).all())
    assert bool((torch.linalg.vector_norm(res.normals.to(F64), dim=1) - 1).abs().max() < 1e-6)
    tri = res.vertices.to(F64)[res.faces.long()]
    geometric = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool(((geometric * (tri.mean(1) - c)).sum(1) > 0).all())
    vol, want = signed_volume(res.vertices - c, res.faces), 4 * np.pi * SPHERE_R ** 3 / 3
    err = (want - vol) / want
    print("sphere: V", V, "E", E, "F", F, "signed volume", vol, "of", want, "short by", err)
    assert vol > 0 and 0 < err <= SPHERE_VOLUME_BOUND, err
    assert MEASURED_SPHERE_VOLUME_ERROR == pytest.approx(err, rel=0.05)
    assert bool((res.weight == 1).all())


# ---- every decision ---------------------------------------------------------------------------------------------------------------------
def cube2(values, w=None):
    """A 2x2x2 volume from eight tsdf values in linear order (x fastest)."""
    return torch.tensor(values, dtype=F32).view(2, 2, 2), torch.ones(2, 2, 2) if w is None else torch.tensor(w, dtype=F32).view(2, 2, 2)


def test_one_positive_corner_is_six_triangles_about_it():
    tsdf, wsum = cube2([1.0] + [-1.0] * 7)
    res = mesh_t(tsdf, wsum, EYE)
    assert res.slots.tolist() == [[0, 0, 0, d] for d in range(7)]          # the seven edges that leave the corner
    assert len(res.faces) == 6 and len(torch.unique(res.faces)) == 7
    want = torch.tensor([[0.5 * v for v in DIRS[d]] for d in range(7)], dtype=F32)
    assert torch.equal(res.vertices, want)
    # the normals point to the positive corner's side
    assert bool(((res.normals * (torch.zeros(3) - res.vertices)).sum(1) > 0).all())
    tri = res.vertices.to(F64)[res.faces.long()]
    geometric = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool(((geometric * (0 - tri.mean(1))).sum(1) > 0).all())        # counter-clockwise seen from the positive side


def test_zeros_are_negative_and_their_triangles_are_kept():
    for zero in (0.0, -0.0):
        tsdf, wsum = cube2([1.0] + [zero] * 7)
        res = mesh_t(tsdf, wsum, EYE)
        assert len(res.vertices) == 7 and len(res.faces) == 6              # a = 1 / (1 - 0) = 1: every vertex at its far end
        assert torch.equal(res.vertices, torch.tensor(DIRS, dtype=F32))
        tsdf, wsum = cube2([zero] + [1.0] * 7)
        res = mesh_t(tsdf, wsum, EYE)
        assert len(res.vertices) == 7 and len(res.faces) == 6 and bool((res.vertices == 0).all())    # a = 0: all at the corner
        assert bool(torch.isfinite(res.normals).all())
    assert len(mesh_t(*cube2([0.0] * 8), EYE).vertices) == 0               # all negative
    assert len(mesh_t(*cube2([-0.0, 0.0] * 4), EYE).faces) == 0


def test_unusable_points():
    base = [1.0] + [-1.0] * 7
    assert len(mesh_t(*cube2(base), EYE).faces) == 6
    for bad in (NAN, INF, -INF):
        for at in (0, 3, 7):
            v = list(base)
            v[at] = bad
            res = mesh_t(*cube2(v), EYE)
            assert len(res.vertices) == 0 and len(res.faces) == 0 and res.vertices.shape == (0, 3) and res.faces.shape == (0, 3), (bad, at)
    above = float(torch.nextafter(torch.tensor(0.5, dtype=F32), torch.tensor(1.0, dtype=F32)))
    for w, n in ((0.5, 0), (above, 6), (NAN, 0), (0.0, 0), (-1.0, 0), (INF, 6)):
        ws = [1.0] * 8
        ws[5] = w
        assert len(mesh_t(*cube2(base, ws), EYE, min_weight=0.5).faces) == n, w      # wsum > min_weight, not >=
    assert len(mesh_t(*cube2(base, [0.5] * 8), EYE, min_weight=0.5).faces) == 0
    assert len(mesh_t(*cube2(base, [0.5] * 8), EYE, min_weight=0.0).faces) == 6
    assert len(mesh_t(*cube2([1.0] * 8), EYE).faces) == 0 and len(mesh_t(*cube2([-1.0] * 8), EYE).vertices) == 0


def test_one_dead_corner_kills_its_cubes_and_no_others():
    tsdf = torch.full((3, 3, 3), -1.0)
    tsdf[1, 1, 1] = 1.0                                                    # the centre positive: a closed surface about it
    wsum = torch.ones(3, 3, 3)
    whole = mesh_t(tsdf, wsum, EYE)
    assert len(unmatched_edges(whole)) == 0 and len(whole.vertices) == 14  # the seven directions, both ways
    V, F = len(whole.vertices), len(whole.faces)
    E = len(np.unique(np.sort(directed_edges(whole.faces), 1), axis=0))
    assert V - E + F == 2 and F == 24
    wsum[0, 0, 0] = 0.0                                                    # kills cube (0, 0, 0) alone
    res = mesh_t(tsdf, wsum, EYE)
    assert len(res.faces) == F - 6 and len(res.vertices) == V - 1          # the body diagonal of that cube lay in it alone
    assert len(unmatched_edges(res)) == 6
    wsum[1, 1, 1] = 0.0                                                    # the centre: every cube is dead
    assert len(mesh_t(tsdf, wsum, EYE).vertices) == 0


def test_every_gradient_fallback():
    # a row along x: ... the gradient at a point takes the central difference, the forward one, the backward one, or 0
    t = torch.tensor([[[3.0, 1.0, -2.0, -7.0]] * 2] * 2, dtype=F32)       # [2,2,4]: no variation along y and z
    usable = np.ones((2, 2, 4), dtype=bool)
    G = _gradient(t.numpy(), usable)
    assert G[0][0, 0].tolist() == [-2.0, -5.0, -8.0, -5.0] and not G[1].any() and not G[2].any()
    usable[0, 0, 0] = False                                                # point 1 loses its lower neighbour: forward
    assert _gradient(t.numpy(), usable)[0][0, 0].tolist()[1] == -3.0
    usable[0, 0, 0], usable[0, 0, 2] = True, False                         # its upper one: backward
    assert _gradient(t.numpy(), usable)[0][0, 0].tolist()[1] == -2.0
    usable[0, 0, 0] = False                                                # both: 0
    assert _gradient(t.numpy(), usable)[0][0, 0].tolist()[1] == 0.0
    # in a mesh: the crossing between x = 1 and x = 2, a = 1/3; n_x = G0 + a (G1 - G0) with G0 = -5, G1 = -8: the normal is -x
    res = mesh_t(t, torch.ones(2, 2, 4), EYE)
    on_x = (res.slots[:, 3] == 0).nonzero()[:, 0]
    assert len(on_x) == 4 and bool((res.normals[on_x] == torch.tensor([-1.0, 0.0, 0.0])).all())
    assert bool((res.vertices[on_x, 0] == torch.tensor(1.0 + 1.0 / 3.0, dtype=F64).to(F32)).all())
    flat = mesh_t(*cube2([1.0] + [-1.0] * 7), torch.zeros(4, 4, dtype=F64))                  # M = 0: len = 0, the normal is +0.0
    assert torch.equal(flat.normals.view(torch.int32), torch.zeros(7, 3, dtype=torch.int32))
    w = torch.ones(2, 2, 4)
    w[:, :, 2:] = 4.0
    assert bool((mesh_t(t, w, EYE).weight[on_x] == 2.0).all())             # 1 + (1/3) (4 - 1)


def test_vertices_are_numbered_by_point_then_direction():
    tsdf, wsum, res = all_cases()
    s = res.slots.numpy()
    nz, ny, nx = tsdf.shape
    key = ((s[:, 2] * ny + s[:, 1]) * nx + s[:, 0]) * 7 + s[:, 3]
    assert bool((np.diff(key) > 0).all())


# ---- mesh.volume_mesh's matrices: T given against T = None followed by the same rigid map ------------------------------------------------
def test_a_pose_is_the_world_mesh_moved():
    tsdf, wsum, _ = all_cases()
    ops = ecm().ops
    origin, voxel = (-0.3, 0.2, 1.5), 0.125
    T = rigid(0.02, -0.03, 0.01, 0.1, -0.2, 0.05)
    S = ops.volume_matrices(EYE, EYE, origin, voxel).C
    assert torch.equal(S, grid_matrix(origin, voxel))
    world, cam = mesh_t(tsdf, wsum, S), mesh_t(tsdf, wsum, ops.volume_matrices(EYE, T, origin, voxel).C)
    assert torch.equal(world.faces, cam.faces) and torch.equal(world.weight, cam.weight)
    moved = world.vertices.to(F64) @ T[:3, :3].T + T[:3, 3]
    assert float((cam.vertices.to(F64) - moved).abs().max()) <= 4 * 2.0 ** -24 * float(moved.abs().max())
    turned = world.normals.to(F64) @ T[:3, :3].T
    assert float((cam.normals.to(F64) - turned).abs().max()) <= 1e-6


# ---- write_ply --------------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """(properties, vertex rows [N, len(properties)] fp32, faces [F,3] int32, the bytes after the header) of a file write_ply wrote."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    nf = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    props = [ln.split()[2] for ln in lines if ln.startswith("property float")]
    assert "property list uchar int vertex_indices" in lines
    body = raw[end:]
    v = np.frombuffer(body[:4 * nv * len(props)], dtype="<f4").reshape(nv, len(props))
    rest = body[4 * nv * len(props):]
    assert len(rest) == 13 * nf
    faces = []
    for k in range(nf):
        n, a, b, c = struct.unpack_from("<Biii", rest, 13 * k)
        assert n == 3
        faces.append((a, b, c))
    return props, v, np.array(faces, dtype=np.int32).reshape(nf, 3), body


def test_write_ply_reads_back_byte_for_byte(tmp_path):
    mesh = ecm().mesh
    _, _, res = all_cases()
    full = mesh.Mesh(res.vertices, res.faces, res.normals, res.weight)
    path = str(tmp_path / "full.ply")
    mesh.write_ply(path, full)
    props, v, f, body = read_ply(path)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert v.tobytes() == torch.cat([res.vertices, res.normals], 1).numpy().tobytes() and f.tobytes() == res.faces.numpy().tobytes()
    # the face block against the packing the writer once had, restated here: one struct.pack per face
    face_block = lambda faces: b"".join(struct.pack("<Biii", 3, a, b, c) for a, b, c in faces.tolist())   # noqa: E731
    assert body[len(v.tobytes()):] == face_block(res.faces) and body == v.tobytes() + face_block(res.faces)
    bare = str(tmp_path / "bare.ply")
    mesh.write_ply(bare, mesh.Mesh(res.vertices, res.faces, None, None))
    props, v, f, body = read_ply(bare)
    assert props == ["x", "y", "z"] and v.tobytes() == res.vertices.numpy().tobytes() and f.tobytes() == res.faces.numpy().tobytes()
    assert body[12 * len(res.vertices):] == face_block(res.faces) and len(res.faces) > 0
    empty = str(tmp_path / "empty.ply")
    mesh.write_ply(empty, mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3), None))
    props, v, f, body = read_ply(empty)
    assert len(v) == 0 and len(f) == 0 and body == b"" == face_block(torch.zeros(0, 3, dtype=torch.int32))
    for bad in ((res.vertices, res.faces), "mesh", None):
        with pytest.raises(ValueError, match="a Mesh"):
            mesh.write_ply(path, bad)
    with pytest.raises(ValueError, match="normals"):
        mesh.write_ply(path, mesh.Mesh(res.vertices, res.faces, res.normals[:-1], None))
    with pytest.raises(ValueError, match="vertices"):
        mesh.write_ply(path, mesh.Mesh(res.vertices[:, :2], res.faces, None, None))


# ---- the op's refusals: all of this runs on CPU tensors ---------------------------------------------------------------------------------
def test_op_signature_and_exports():
    e = ecm()
    mesh = e.mesh
    sig = inspect.signature(mesh.volume_mesh)
    assert list(sig.parameters) == ["tsdf", "wsum", "origin", "voxel", "T", "min_weight", "with_normals", "with_weight"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [None, 0.0, True, False]
    assert mesh.Mesh._fields == ("vertices", "faces", "normals", "weight")
    assert list(inspect.signature(mesh.write_ply).parameters) == ["path", "mesh"]
    sig = inspect.signature(e.models.StereoMapper.mesh)
    assert list(sig.parameters) == ["self", "min_weight", "kw"] and sig.parameters["min_weight"].default == 0.0
    import importlib
    pkg = importlib.import_module("explicit-context-mapping-for-stereo-matching_amd")
    assert pkg.__all__[-1] == "mesh" and pkg.mesh is mesh and "ops" in pkg.__all__
    assert mesh.mesh_tile() == TILE and mesh.mesh_brick() == BRICK


def test_volume_mesh_refusals():
    mesh = ecm().mesh
    origin, voxel = (0.0, 0.0, 1.0), 0.1
    vol = lambda *d: (fake(*d), fake(*d))                                                        # noqa: E731
    run = lambda t=None, w=None, origin=origin, voxel=voxel, **kw: mesh.volume_mesh(             # noqa: E731
        *(vol(3, 4, 5) if t is None else (t, w)), origin, voxel, **kw)
    for bad in (-1.0, NAN, INF, True, "w", None, 1e39):
        with pytest.raises(ValueError, match="min_weight"):
            run(min_weight=bad)
    for bad in ((0.0, 1.0), (0.0, 1.0, NAN), "abc", None):
        with pytest.raises(ValueError, match="origin"):
            run(origin=bad)
    for bad in (0.0, -1.0, NAN, INF, True):
        with pytest.raises(ValueError, match="voxel"):
            run(voxel=bad)
    scaled, mirrored = torch.eye(4, dtype=F64), torch.eye(4, dtype=F64)
    scaled[:3, :3] *= 1.001
    mirrored[0, 0] = -1.0
    for bad in (scaled, mirrored):
        with pytest.raises(ValueError, match="not rigid"):
            run(T=bad)
    for bad in (torch.eye(4), torch.eye(3, dtype=F64), "T", torch.full((4, 4), NAN, dtype=F64)):
        with pytest.raises(ValueError, match="T"):
            run(T=bad)
    with pytest.raises(ValueError, match="one \\[4,4\\] matrix"):
        run(T=torch.stack([torch.eye(4, dtype=F64)] * 2))
    # the planes, in _volume_planes' words
    g = torch.zeros(3, 4, 5, requires_grad=True)
    for call in (lambda: run(g, fake(3, 4, 5)), lambda: run(fake(3, 4, 5), g)):
        with pytest.raises(ValueError, match="requires grad"):
            call()
    with pytest.raises(RuntimeError, match="CPU tensor"):
        run(torch.ones(3, 4, 5), torch.zeros(3, 4, 5))
    with pytest.raises(RuntimeError, match="contiguous"):
        run(fake(3, 5, 4).transpose(1, 2), fake(3, 4, 5))
    one = fake(3, 4, 5)
    with pytest.raises(RuntimeError, match="one tensor"):
        run(one, one)
    for dims in ((1, 4, 5), (3, 1, 5), (3, 4, 1)):
        with pytest.raises(RuntimeError, match="every dim >= 2"):
            run(*vol(*dims))
    for t, w in ((fake(3, 4, 5), fake(3, 4, 6)), (fake(4, 5), fake(4, 5)), (fake(3, 4, 5, dtype=F64), fake(3, 4, 5, dtype=F64))):
        with pytest.raises(RuntimeError):
            run(t, w)
    with pytest.raises(ValueError, match="a tensor"):
        run("tsdf", fake(3, 4, 5))
    with pytest.raises(RuntimeError, match="at most 2\\^27"):
        run(*vol(2, 1 << 14, (1 << 12) + 1))                               # fake() allocates nothing
    e = ecm()
    mapper = e.models.StereoMapper(e.get_model("cmfsm"), e.ops.q_matrix(700.0, 0.25, 64.0, 32.0), (-1.0, -1.0, 0.5), 0.05, (8, 8, 8), 0.2)
    with pytest.raises(ValueError, match="no frame"):
        mapper.mesh()


# ---- the census of the seventh header -----------------------------------------------------------------------------------------------------
def header_prototypes():
    with open(os.path.join(INCLUDE, HEADER)) as f:
        return parse_header(f.read())


def test_the_registries():
    lib = ecm()._lib
    assert lib.REGISTRIES == (lib.TABLES, lib.EXTENSION_TABLES, lib.MOTION_TABLES) and lib.LATER_REGISTRIES == (lib.VOLUME_TABLES,)
    assert tuple(lib.TABLES) == ("ecm_hip.h", "ecm_geometry.h", "ecm_rectify.h") and tuple(lib.EXTENSION_TABLES) == ("ecm_temporal.h",)
    assert tuple(lib.MOTION_TABLES) == ("ecm_motion.h",) and tuple(lib.VOLUME_TABLES) == ("ecm_volume.h",)
    before = dict(lib._all_tables())
    assert len(before) == sum(len(t) for reg in lib.REGISTRIES + lib.LATER_REGISTRIES for t, _ in reg.values())
    assert not any(n in before for n in ENTRIES)
    assert lib.NEWER_REGISTRIES == (lib.MESH_TABLES,) and tuple(lib.MESH_TABLES) == (HEADER,)
    assert lib.MESH_TABLES[HEADER][0] is lib.MESH_PROTOTYPES and lib.MESH_TABLES[HEADER][1] == PREFIX
    every = dict(lib._every_table())
    assert len(every) == len(before) + len(ENTRIES) and all(n in every for n in ENTRIES) and all(every[n] == before[n] for n in before)


def test_header_table_and_package_literals_name_the_same_entries():
    lib = ecm()._lib
    parsed = header_prototypes()
    with open(os.path.join(INCLUDE, HEADER)) as f:
        by_text = set(re.findall(rf"\b({PREFIX}[a-z0-9_]+)\s*\(", _strip(f.read())))
    found = package_entry_names(PREFIX + "[a-z0-9_]+", "MESH_PROTOTYPES")
    assert sorted(parsed) == sorted(by_text) == sorted(lib.MESH_PROTOTYPES) == sorted(found) == sorted(ENTRIES)
    assert all(n.startswith(PREFIX) for n in parsed)
    assert all(a.startswith("mesh.py:") for at in found.values() for a in at), found
    for registry in lib.REGISTRIES + lib.LATER_REGISTRIES:
        for table, _ in registry.values():
            assert not set(table) & set(lib.MESH_PROTOTYPES)


def test_prototypes_match_the_header_type_by_type():
    table, parsed = ecm()._lib.MESH_PROTOTYPES, header_prototypes()
    assert compare(parsed, table) == []
    assert all(table[n] == parsed[n] for n in parsed)


def test_library_exports_every_row_and_load_types_it(lib_mod):
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in ENTRIES if not hasattr(lib, n)] == [] and lib_mod.missing_symbols() == []
    table = lib_mod.MESH_PROTOTYPES
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
    assert lib_mod.query("ecms_mesh_tile") == TILE and tuple(lib_mod.query("ecms_mesh_brick", a) for a in range(3)) == BRICK
    assert lib_mod.query("ecms_mesh_brick", 3) == 0 and lib_mod.query("ecms_mesh_brick", -1) == 0


def scratch_bytes(nx, ny, nz):
    """The header's formula."""
    P = nx * ny * nz
    return (8 * P + 8 * ((P + TILE - 1) // TILE) + 15) // 16 * 16


def test_scratch_bytes_is_the_headers_formula(lib_mod):
    q = lambda *a: lib_mod.query("ecms_mesh_scratch_bytes", *a)                                  # noqa: E731
    for dims in ((2, 2, 2), (6, 7, 8), (16, 4, 4), (17, 5, 5), (2048, 2, 2), (2049, 2, 2), (512, 512, 512), (1 << 25, 2, 2)):
        assert q(*dims) == scratch_bytes(*dims), dims
    for dims in ((1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 2, 2), (-1, 2, 2), (513, 512, 512), (1 << 26, 2, 2), (1 << 30, 1 << 30, 1 << 30),
                 (2147483647, 2147483647, 2147483647)):
        assert q(*dims) == 0, dims


# ---- the refusal contract, with the devices hidden --------------------------------------------------------------------------------------
SMALL = scratch_bytes(2, 2, 2)
LARGEST = {"nx": 512, "ny": 512, "nz": 512, "scratch_bytes": scratch_bytes(512, 512, 512)}       # 2^27 points exactly
TOO_LARGE = [{"nx": 513, "ny": 512, "nz": 512, "scratch_bytes": 1 << 40}, {"nx": 1 << 26, "scratch_bytes": 1 << 40},
             {"nx": 65536, "ny": 65536, "scratch_bytes": 1 << 40}]
ROWS = [
    # a short scratch is ECM_EINVAL here ("scratch_bytes below ecms_mesh_scratch_bytes"), so scratch_bytes is a size of the row: 0 and
    # -1 are probed, one byte short is named, and the query's own value is legal
    Row("ecms_mesh_count_fwd", f"tsdf:p wsum:p counts:p scratch:p scratch_bytes=L{SMALL} nx=2 ny=2 nz=2 min_weight=f0 stream:s",
        inval=[{"nx": 1}, {"ny": 1}, {"nz": 1}, {"scratch_bytes": SMALL - 1}, {"nx": 3, "ny": 3, "nz": 3}],
        legal=[{"scratch_bytes": SMALL + 1}, {"nx": 3, "ny": 3, "nz": 3, "scratch_bytes": scratch_bytes(3, 3, 3)}, LARGEST],
        unsup=TOO_LARGE, header=HEADER),
    Row("ecms_mesh_emit_fwd",
        f"tsdf:p wsum:p M:p vertices:p faces:p normals:o weight:o scratch:p scratch_bytes=L{SMALL} n_vertices=-L4 n_faces=-L4 nx=2 ny=2 "
        "nz=2 min_weight=f0 stream:s",
        inval=[{"nx": 1}, {"ny": 1}, {"nz": 1}, {"scratch_bytes": SMALL - 1}, {"nx": 3, "ny": 3, "nz": 3}],
        legal=[{"n_vertices": 0}, {"n_faces": 0}, {"n_vertices": 1 << 40, "n_faces": 1 << 40}, LARGEST],
        unsup=TOO_LARGE, header=HEADER),
]
INT_CONSTS = ("ecms_mesh_tile",)


@pytest.fixture(scope="module")
def results(lib_mod):
    """{call id: return value} of the rows above from one fresh child that sees no device (tests/abi_refusal_child.py)."""
    parsed = header_prototypes()
    calls = [{"id": f"const|{n}", "fn": n, "res": "i", "args": []} for n in INT_CONSTS]
    for row in ROWS:
        calls += calls_of(row, lambda q: parsed[q][1])
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


def test_every_entry_of_the_seventh_header_has_a_row():
    parsed = header_prototypes()
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    assert sorted(ent) == sorted(r.name for r in ROWS) and sorted(qry) == ["ecms_mesh_scratch_bytes"]
    for r in ROWS:
        assert r.types == ent[r.name], r.name
    assert sorted(set(parsed) - set(ent) - set(qry)) == ["ecms_mesh_brick", "ecms_mesh_tile"]


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    row = next(r for r in ROWS if r.name == name)
    bad = classify(row, results)
    assert not bad, "\n" + _report(bad)
    assert results[f"{name}|accepted"] > 0                                 # the pointers are never dereferenced: no device, no crash
    assert results["const|ecms_mesh_tile"] == TILE


def test_further_refusals_of_the_entries(lib_mod):
    """What the rows cannot express: floats, and an output that is an input or another output.  Every call returns before any HIP
    call."""
    lib = lib_mod.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(10)]                    # never dereferenced
    base = [("tsdf", p[0]), ("wsum", p[1]), ("counts", p[2]), ("scratch", p[3]), ("bytes", C.c_longlong(SMALL)), ("nx", 2), ("ny", 2),
            ("nz", 2), ("min_weight", 0.0), ("stream", None)]
    call = lambda **kw: lib.ecms_mesh_count_fwd(*[kw.get(k, v) for k, v in base])                # noqa: E731
    for out in ("counts", "scratch"):
        for i in range(2):
            assert call(**{out: p[i]}) == EINVAL, (out, i)
    assert call(scratch=p[2]) == EINVAL
    for bad in (-1.0, -1e-30, NAN, INF, -INF):
        assert call(min_weight=bad) == EINVAL, bad
    assert call(nx=513, ny=512, nz=512) == EUNSUP and call(nx=513, ny=512, nz=512, min_weight=NAN) == EINVAL
    names = ("tsdf", "wsum", "M")
    outs = ("vertices", "faces", "normals", "weight", "scratch")
    base = [(n, p[i]) for i, n in enumerate(names)] + [(n, p[3 + i]) for i, n in enumerate(outs)] + [
        ("bytes", C.c_longlong(SMALL)), ("nv", C.c_longlong(4)), ("nf", C.c_longlong(4)), ("nx", 2), ("ny", 2), ("nz", 2),
        ("min_weight", 0.0), ("stream", None)]
    call = lambda **kw: lib.ecms_mesh_emit_fwd(*[kw.get(k, v) for k, v in base])                 # noqa: E731
    for out in outs:
        for i, n in enumerate(names):
            assert call(**{out: p[i]}) == EINVAL, (out, n)
    for i, a in enumerate(outs):
        for b in outs[i + 1:]:
            assert call(**{b: p[3 + i]}) == EINVAL, (a, b)
    for bad in (-1.0, NAN, INF):
        assert call(min_weight=bad) == EINVAL, bad
    assert call(nv=C.c_longlong(-1)) == EINVAL and call(nf=C.c_longlong(-1)) == EINVAL
    assert call(nx=513, ny=512, nz=512) == EUNSUP
    # no legal call is made here: this process may see a device, and the pointers are not device memory
