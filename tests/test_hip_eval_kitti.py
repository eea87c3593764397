"""ops.eval_kitti (csrc/eval.hip `ecm_eval_kitti`) and dist.evaluate_kitti on the MI355X: the reference's eval_kitti.py:84-115.

Checks.
  * Discrete results -- the four counts -- equal the fp32 decisions of the statements (test_eval_kitti_cpu.restate64) exactly, and
    loss_3 equals 100 - good / total * 100 formed in fp32 from them (the reference's three roundings) bit for bit.
  * Continuous results -- the three means -- against the fp64 sum over the same selections under the yardstick of
    tests/test_hip_metrics_fp64.py (imported): |hip - q64| <= K * e32 + FLOOR * max|q64|, e32 the larger error of the reference's torch
    statements on the CPU and on the device.  Each check prints a `CVRATIO` line.
  * Every run goes through guard bands around out8, the table and the scratch (test_hip_guard_bands.guarded), over an allocator whose
    free blocks hold NaN, twice on fresh operands, and must repeat bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_eval_kitti_cpu as R
from conftest import load_golden
from test_hip_conv3d_fp64 import DEV, FLOOR, K
from test_hip_costvol_fp64 import off4, poison
from test_hip_guard_bands import guarded
from test_hip_metrics_fp64 import yardstick

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run_once(ecm, pred, gt, place=lambda t: t.to(DEV)):
    poison()
    with guarded(ecm) as g:
        row, table = ecm.ops.eval_kitti(place(pred), place(gt), R.MAXDISP, per_sample=True)
        g.check("eval_kitti")
        assert len(g.records) == 3                       # out8, the table, the scratch
        return row.clone(), table.clone()


def run(ecm, pred, gt, place=lambda t: t.to(DEV)):
    """Twice on fresh operands; -> (row [8], table [B,8]) on the CPU."""
    a, b = run_once(ecm, pred, gt, place), run_once(ecm, pred, gt, place)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), "two runs differ"
    ecm.ops.check_async_errors()
    return a[0].cpu(), a[1].cpu()


def check_row(path, name, got, pred, gt, fails, draws=None):
    """One row of eight against the statements over (pred, gt)."""
    want = R.restate64(pred, gt)
    print(f"CVCOUNT {path} counts {[int(v) for v in got[4:]]} / {[int(v) for v in want[4:]]}   # {name}")
    if got[4:].double().tolist() != want[4:].tolist():
        fails.append(f"{name}: counts {got[4:].tolist()} != {want[4:].tolist()}")
    if not (float(got[3]) == want[3] or (np.isnan(want[3]) and bool(torch.isnan(got[3])))):
        fails.append(f"{name}: loss_3 {float(got[3])!r} != {want[3]!r}")
    if not np.isnan(want[:3]).all():
        draws = draws or [R.torch_statements(pred, gt, "cpu"), R.torch_statements(pred, gt, DEV)]
    for k in range(3):
        if np.isnan(want[k]):
            if not bool(torch.isnan(got[k])):
                fails.append(f"{name}: {R.COLUMNS[k]} over an empty selection is {float(got[k])}, not NaN")
            continue
        yardstick(path, name, R.COLUMNS[k], got[k], want[k], [d[k] for d in draws], fails)
    if not torch.equal(bits(got[[1, 5]]), bits(got[[2, 6]])):
        fails.append(f"{name}: the mask_true columns differ from the mask_non columns")
    return want


def random_case(B, H, W, seed):
    """Off-grid values (the sums round): d in [-20, 240) with zeros sprinkled in, as sparse ground truth has; p = d + N(0, 2.5)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, H, W, generator=g) * 260.0 - 20.0
    gt[torch.rand(B, H, W, generator=g) < 0.3] = 0.0
    gt[..., W // 2:] *= 0.25                                  # x - d >= 0 on a good share of the right half
    pred = gt + torch.randn(B, H, W, generator=g) * 2.5
    return pred, gt


# ---- fixture parity ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES)
def test_fixture_parity(ecm, case):
    g = load_golden("g14_eval_kitti")
    pred, gt = g[case + ".pred"], g[case + ".gt"]
    ref_loss, ref_count = g[case + ".loss"], g[case + ".count"]
    row, table = run(ecm, pred, gt)
    fails = []
    check_row("kitti.fixture", case, row, pred, gt, fails)
    assert row[[4, 5, 6, 7]].long().tolist() == ref_count.tolist()
    if case == "empty":
        assert torch.isnan(row[:4]).all() and torch.isnan(table[:, :4]).all() and not table[:, 4:].any()
    else:
        ulp = float(np.spacing(np.float32(ref_loss[3])))
        print(f"CVULP kitti.fixture loss_3 {abs(float(row[3]) - float(ref_loss[3])) / ulp:.1f}   # {case}")
        assert abs(float(row[3]) - float(ref_loss[3])) <= ulp
    assert not fails, "\n".join(fails)


# ---- decision boundaries -----------------------------------------------------------------------------------------------------

def test_decision_boundaries(ecm):
    pred, gt = R.boundary_table()
    rows = R.boundary_rows()
    row, _ = run(ecm, pred, gt)
    n, n_non, n_good = sum(r[3] for r in rows), sum(r[4] for r in rows), sum(r[5] for r in rows)
    assert row[4:].tolist() == [n, n_non, n_non, n_good]
    fails = []
    check_row("kitti.boundary", "boundary_table", row, pred, gt, fails)
    # one boundary pixel at a time: a wrong decision cannot hide behind another one
    for x, d, p, in_mask, in_non, good in rows:
        one_p, one_d = torch.full((1, 1, 208), 7.0), torch.zeros(1, 1, 208)
        one_p[0, 0, x], one_d[0, 0, x] = p, d
        got = ecm.ops.eval_kitti(one_p.to(DEV), one_d.to(DEV)).cpu()
        assert got[4:].tolist() == [float(in_mask), float(in_non), float(in_non), float(good)], f"column {x}, d {d!r}, p {p!r}"
        if in_mask:
            assert float(got[0]) == abs(p - d) and float(got[3]) == (0.0 if good else 100.0), f"column {x}"
    assert not fails, "\n".join(fails)


def test_nan_prediction_under_the_mask(ecm):
    """The reference: |NaN - d| = NaN goes into the mean (NaN), both comparisons of error_map are false (not good), and the pixel
    counts in `total`.  A NaN outside the mask touches nothing."""
    pred, gt = random_case(2, 9, 52, 5)
    gt[0, 3, 40], gt[1, 2, 3], gt[0, 0, 0] = 10.0, 100.0, 0.0          # in mask and mask_non; in mask only; outside
    clean = R.restate64(pred, gt)
    pred[0, 3, 40] = pred[1, 2, 3] = pred[0, 0, 0] = float("nan")
    row, table = run(ecm, pred, gt)
    want = R.restate64(pred, gt)
    ref = R.torch_statements(pred, gt, "cpu")
    assert torch.isnan(ref[:3]).all() and float(ref[3]) == want[3]
    assert torch.isnan(row[:3]).all() and torch.isnan(table[:, 0]).all() and torch.isnan(table[0, 1]) and not torch.isnan(table[1, 1])
    assert row[4:].double().tolist() == want[4:].tolist() and float(row[3]) == want[3]
    assert want[7] <= clean[7] and want[4] == clean[4]


# ---- reduction-grid edges ----------------------------------------------------------------------------------------------------

GRID = {   # name: (B, H, W)
    "tiny": (1, 1, 7),                                    # fewer pixels than one workgroup
    "span_minus_1": (3, 23, 89),                          # 2047: a ragged only block; samples do not start on a 16-byte boundary
    "span": (3, 8, 256),                                  # 2048: exactly one block per sample, 16-byte loads
    "span_plus_1": (3, 3, 683),                           # 2049: a second block with one pixel
    "span_plus_4_vec": (2, 1, 2052),                      # ... and with one float4
    "b33": (33, 23, 89),
    "cap": (1, 512, 1024),                                # 256 blocks of 2048: the cap, reached
    "past_cap": (1, 514, 1024),                           # 257 spans: block 0 walks two of them
    "past_cap_scalar": (1, 2, 262145),                    # 256 spans + 2 pixels, W % 4 != 0
}


@pytest.mark.parametrize("name", sorted(GRID))
def test_reduction_grid(ecm, name):
    B, H, W = GRID[name]
    pred, gt = random_case(B, H, W, seed=len(name) + H)
    row, table = run(ecm, pred, gt)
    fails = []
    path = "kitti.%s.%dwg" % ("vec" if W % 4 == 0 else "scalar", R.kitti_blocks(H * W))
    check_row(path, name, row, pred, gt, fails)
    for b in sorted({0, B // 2, B - 1}):
        check_row(path, f"{name}[{b}]", table[b], pred[b:b + 1], gt[b:b + 1], fails)
    assert table[:, 4:].double().sum(0).tolist() == row[4:].double().tolist(), "the rows' counts do not add up to the batch row"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [(2, 8, 256), (1, 6, 1028)])
def test_scalar_path_on_the_same_data(ecm, shape):
    """A view 4 bytes past a 16-byte boundary takes the scalar path; the vector path on the same values: identical counts (and
    loss_3), means that differ by summation order only."""
    pred, gt = random_case(*shape, seed=11)
    vec, vec_t = run(ecm, pred, gt)
    aligned = lambda t: t.to(DEV)
    for place in ((off4, aligned), (aligned, off4), (off4, off4)):
        poison()
        with guarded(ecm) as g:
            sca, sca_t = ecm.ops.eval_kitti(place[0](pred), place[1](gt), per_sample=True)
            g.check("eval_kitti scalar")
        sca, sca_t = sca.cpu(), sca_t.cpu()
        assert torch.equal(bits(sca[3:]), bits(vec[3:])) and torch.equal(bits(sca_t[:, 3:]), bits(vec_t[:, 3:]))
        fails = []
        check_row("kitti.scalar.off4", str(shape), sca, pred, gt, fails)
        assert not fails, "\n".join(fails)


# ---- per-sample table --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 23, 89), (3, 8, 256), (4, 3, 2052)])
def test_per_sample_table(ecm, shape):
    B = shape[0]
    pred, gt = random_case(*shape, seed=21)
    gt[1] = torch.tensor([0.0, 192.0, 200.0, -1.0]).repeat(shape[1] * shape[2] // 4 + 1)[:shape[1] * shape[2]].view(shape[1:])
    row, table = run(ecm, pred, gt)
    pd, gd = pred.to(DEV), gt.to(DEV)
    for b in range(B):
        alone = ecm.ops.eval_kitti(pd[b:b + 1], gd[b:b + 1])
        assert torch.equal(bits(alone), bits(table[b])), f"row {b} is not the op on sample {b} alone"
    assert table[:, 4:].double().sum(0).tolist() == row[4:].double().tolist()
    assert torch.isnan(table[1, :4]).all() and not table[1, 4:].any()
    assert not torch.isnan(table[[0] + list(range(2, B))]).any() and not torch.isnan(row).any()
    no_table = ecm.ops.eval_kitti(pd.unsqueeze(1), gd)                       # [B,1,H,W]; NULL per_sample
    assert torch.equal(bits(no_table), bits(row))


# ---- out= ----------------------------------------------------------------------------------------------------------------------

def test_out_row_of_a_log(ecm):
    pred, gt = random_case(2, 23, 89, seed=31)
    pd, gd = pred.to(DEV), gt.to(DEV)
    want = ecm.ops.eval_kitti(pd, gd).clone()
    assert not torch.isnan(want).any()
    log = torch.full((5, 8), float("nan"), device=DEV)
    before = bits(log)
    ret, table = ecm.ops.eval_kitti(pd, gd, out=log[2], per_sample=True)
    assert ret.data_ptr() == log[2].data_ptr() and table.shape == (2, 8)
    after = bits(log)
    assert torch.equal(after[[0, 1, 3, 4]], before[[0, 1, 3, 4]]) and torch.equal(after[2], bits(want))
    for bad in (log[:, 0], log[2, :7], torch.zeros(8), log[2].double()):
        with pytest.raises(RuntimeError):
            ecm.ops.eval_kitti(pd, gd, out=bad)

    want6 = ecm.ops.eval_epe(pd, gd, 20, 80).clone()
    log6 = torch.full((5, 6), float("nan"), device=DEV)
    before = bits(log6)
    ret = ecm.ops.eval_epe(pd, gd, 20, 80, out=log6[4])
    after = bits(log6)
    assert ret.data_ptr() == log6[4].data_ptr()
    assert torch.equal(after[:4], before[:4]) and torch.equal(after[4], bits(want6)) and not torch.isnan(want6).any()


def test_undersized_scratch(ecm):
    B, H, W = 2, 23, 89
    nb = ecm._lib.query("ecm_eval_kitti_scratch_bytes", B, H, W)
    assert nb == R.scratch_bytes(B, H, W)
    pd, gd = (t.to(DEV) for t in random_case(B, H, W, seed=41))
    out, scratch = torch.zeros(8, device=DEV), torch.zeros(nb, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        ecm._lib.call("ecm_eval_kitti", p(pd), p(gd), p(out), C.c_void_p(0), p(scratch), C.c_longlong(nb - 1), B, H, W,
                      C.c_float(R.MAXDISP), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert not out.any() and not scratch.any()
    with pytest.raises(RuntimeError):
        ecm.ops.eval_kitti(pd, gd[:, :, :-1])


# ---- KITTI size ------------------------------------------------------------------------------------------------------------------

def test_kitti_frame_size(ecm):
    """384 x 1248 at B = 2 with the ground truth zeroed at the top and left as ops.frame_prep_kitti_eval leaves it for a 375 x 1242 frame."""
    pred, gt = random_case(2, 384, 1248, seed=51)
    gt[:, :9, :], gt[:, :, :6] = 0.0, 0.0
    row, table = run(ecm, pred, gt)
    fails = []
    draws = [R.torch_statements(pred, gt, "cpu"), R.torch_statements(pred, gt, DEV)]
    check_row("kitti.vec.234wg", "kitti_384x1248", row, pred, gt, fails, draws)
    assert float(row[3]) == float(draws[0][3]) == float(draws[1][3])
    check_row("kitti.vec.234wg", "kitti_384x1248[1]", table[1], pred[1:], gt[1:], fails)
    assert not fails, "\n".join(fails)


# ---- dist.evaluate_kitti -------------------------------------------------------------------------------------------------------

class Stub(torch.nn.Module):
    """`left` carries the prediction: output3 = left[:, :1]; the other two heads are decoys."""

    def forward(self, left, right):
        assert not self.training and not torch.is_grad_enabled()
        o3 = left[:, :1]
        return o3 * 0.5, o3 * 0.7, o3


def bound(ref, draws):
    return K * max(abs(float(d) - ref) for d in draws) + FLOOR * abs(ref)


def test_evaluate_kitti(ecm, tmp_path):
    import torch.distributed as dist
    from importlib import import_module
    D = import_module("explicit-context-mapping-for-stereo-matching_amd.dist")
    pred, gt = random_case(5, 24, 40, seed=61)
    pd, gd = pred.to(DEV), gt.to(DEV)
    batches = [(pd[i:j].unsqueeze(1), torch.zeros(j - i, 1, 24, 40, device=DEV), gd[i:j], None) for i, j in ((0, 2), (2, 4), (4, 5))]
    model = Stub().train()
    res = D.evaluate_kitti(model, batches)
    assert not model.training and res["log"].shape == (3, 8) and res["per_sample"].shape == (5, 8)
    assert "per_sample_all" not in res
    for key, col in (("", 0), ("_non", 1), ("_true", 2), ("_3", 3)):
        rec = res["error_rec" + key]
        assert isinstance(rec, list) and len(rec) == 3 and all(isinstance(v, float) for v in rec)
        assert res["error" + key] == np.mean(rec)
        want_mean, slack = [], []
        for n, (i, j) in enumerate(((0, 2), (2, 4), (4, 5))):
            q64 = R.restate64(pred[i:j], gt[i:j])[col]
            draws = [R.torch_statements(pred[i:j], gt[i:j], dev)[col] for dev in ("cpu", DEV)]
            want_mean.append(float(draws[0]))
            if col == 3:
                assert rec[n] == q64 == float(draws[0]) == float(draws[1])
            else:
                slack.append(bound(q64, draws) + abs(float(draws[0]) - q64))
                print(f"CVRATIO kitti.loop error_rec{key}[{n}] {abs(rec[n] - q64) / bound(q64, draws):.3f}")
                assert abs(rec[n] - q64) <= bound(q64, draws)
        # the reference's figure: np.mean over its own `.item()` list
        assert abs(res["error" + key] - np.mean(want_mean)) <= (np.mean(slack) if slack else 0.0)
    for b in range(5):
        assert torch.equal(bits(res["per_sample"][b]), bits(ecm.ops.eval_kitti(pd[b:b + 1], gd[b:b + 1])))

    all64 = R.restate64(pred, gt)
    draws = [R.torch_statements(pred, gt, dev) for dev in ("cpu", DEV)]
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        res1 = D.evaluate_kitti(Stub(), batches)
    finally:
        dist.destroy_process_group()
    assert torch.equal(bits(res1["per_sample_all"]), bits(res["per_sample"])) and res1["error_rec"] == res["error_rec"]
    for ds in (res1["dataset"], res["dataset"]):
        assert [ds[k] for k in R.COLUMNS[4:]] == all64[4:].tolist()
        assert ds["loss_3"] == 100.0 - all64[7] / all64[4] * 100.0
        for k in range(3):
            print(f"CVRATIO kitti.dataset {R.COLUMNS[k]} {abs(ds[R.COLUMNS[k]] - all64[k]) / bound(all64[k], [d[k] for d in draws]):.3f}")
            assert abs(ds[R.COLUMNS[k]] - all64[k]) <= bound(all64[k], [d[k] for d in draws])
