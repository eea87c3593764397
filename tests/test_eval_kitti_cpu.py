"""The KITTI validation leg (eval_kitti.py:84-103; csrc/eval.hip `ecm_eval_kitti`, ops.eval_kitti) as far as it can be checked without
a GPU, and the helpers tests/test_hip_eval_kitti.py shares:

  * `restate64`: the statements restated -- every decision (the masks, `good`) and |p - d| in fp32 as the reference takes them, the
    sums over those selections in fp64.  It must reproduce every case of fixture g14 (the reference's own outputs): counts exactly,
    loss_3 (formed in fp32 from the counts, as the reference does) exactly, means within the fp32 rounding of the stored values.
  * `torch_statements`: the same statements in torch fp32 on a device of choice (the "e32 draws" of the GPU yardstick).
  * `boundary_table`: one pixel per decision boundary, every fp32 difference exact (shown here on the CPU)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_abi_types import declared

MAXDISP = 192.0
COLUMNS = ("loss", "loss_non", "loss_true", "loss_3", "n_mask", "n_non", "n_true", "n_good")
CASES = ("b2", "b1", "empty", "sample_empty")
KT, KSPAN, KITTI_MAX_BLOCKS, KP = 256, 2048, 256, 5        # csrc/eval.hip


def kitti_blocks(hw):
    return min(KITTI_MAX_BLOCKS, -(-hw // KSPAN))


def scratch_bytes(B, H, W):
    return -(-B * kitti_blocks(H * W) * KP * 4 // 8) * 8 + B * KP * 8


def decisions(pred, gt, maxdisp=MAXDISP):
    """fp32, as the reference: (e, mask, mask_non, good under mask)."""
    pred, gt = pred.float().reshape(gt.shape), gt.float()
    x = torch.arange(gt.shape[-1], dtype=torch.float32).expand_as(gt)
    mask = (gt < maxdisp) & (gt > 0)
    non = mask & ((x - gt) >= 0)
    e = (pred - gt).abs()
    good = mask & ((e < 3) | (e < torch.tensor(0.05, dtype=torch.float32) * gt))
    return e, mask, non, good


def err3_fp32(n_good, n_mask):
    """100 - good / total * 100 with fp32 operands and three fp32 roundings (eval_kitti.py:103); 0 / 0 -> NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float32(100) - np.float32(n_good) / np.float32(n_mask) * np.float32(100))


def restate64(pred, gt, maxdisp=MAXDISP):
    """-> float64[8] in COLUMNS order: means summed in fp64 over the fp32 decisions; NaN for an empty selection."""
    e, mask, non, good = decisions(pred, gt, maxdisp)
    e = e.double()
    n, n_non, n_good = int(mask.sum()), int(non.sum()), int(good.sum())
    m = float(e[mask].sum()) / n if n else float("nan")
    m_non = float(e[non].sum()) / n_non if n_non else float("nan")
    return np.array([m, m_non, m_non, err3_fp32(n_good, n), n, n_non, n_non, n_good], dtype=np.float64)


def torch_statements(pred, gt, device, maxdisp=MAXDISP):
    """The reference's statements in torch fp32 on `device` -> float32[4] tensor (loss, loss_non, loss_true, loss_3) on the CPU;
    `.tolist()` at the end stands for its three `.item()` calls."""
    d, o = gt.to(device), pred.to(device).reshape(gt.shape)
    ones, zeros = torch.ones(1, device=device), torch.zeros(1, device=device)
    x = torch.arange(d.shape[-1], device=device).float().expand_as(d)
    mask = (d < maxdisp) & (d > 0)
    non = mask & ((x - d) >= 0)
    e = torch.abs(o[mask] - d[mask])
    loss = torch.mean(e)
    loss_non = torch.mean(torch.abs(o[non] - d[non]))
    loss_true = torch.mean(torch.abs(o[non] - d[non]))
    good = torch.where((e < 3) | (e < 0.05 * d[mask]), ones, zeros)
    total = torch.where(d[mask] > 0, ones, zeros)
    loss_3 = 100 - torch.sum(good) / torch.sum(total) * 100
    return torch.tensor([loss.item(), loss_non.item(), loss_true.item(), loss_3.item()])


def _f32(v):
    return float(np.float32(v))


def below(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def above(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def boundary_rows():
    """(column x, d, p, in mask, in mask_non, good): one pixel per side of every decision of the kernel.  p is chosen so that
    p - d is exact in fp32 (both within a factor 2 of each other, or small dyadic numbers)."""
    t64 = _f32(np.float32(0.05) * np.float32(64.0))                 # 3.2000000477: e must pass 3 first, so only 0.05f * d decides
    k = int(t64 / 2.0 ** -18)                                       # e = k * 2^-18 < t64 < (k + 1) * 2^-18, p = 64 - e near 60.8
    assert k * 2.0 ** -18 < t64 < (k + 1) * 2.0 ** -18
    assert _f32(np.float32(0.05) * np.float32(100.0)) == 5.0
    return [
        (0, 0.0, 1.0, False, False, False),                         # d == 0
        (1, -0.5, 0.0, False, False, False),                        # d < 0
        (2, 192.0, 192.0, False, False, False),                     # d == maxdisp
        (3, below(192.0), 191.0, True, False, True),                # its fp32 neighbour below: in the mask, x - d < 0
        (200, below(192.0), 191.0, True, True, True),               # ... and with x - d >= 0
        (4, 4.0, 4.5, True, True, True),                            # x - d == 0
        (5, above(5.0), 5.5, True, False, True),                    # one ulp past it
        (6, below(6.0), 6.5, True, True, True),                     # one ulp before it
        (10, 1.0, 4.0, True, True, False),                          # e == 3 (0.05f * d = 0.05 decides nothing)
        (11, 1.0, below(4.0), True, True, True),                    # e == 3 - 2^-22
        (12, 1.0, -above(2.0), True, True, False),                  # e == 3 + 2^-22, p below d
        (101, 100.0, 95.0, True, True, False),                      # e == 0.05f * 100 == 5: not below it
        (102, 100.0, above(95.0), True, True, True),                # e == 5 - 2^-17: only the 5 % test passes
        (103, 100.0, 106.0, True, True, False),
        (70, 64.0, 64.0 - k * 2.0 ** -18, True, True, True),        # the largest e below 0.05f * 64
        (71, 64.0, 64.0 - (k + 1) * 2.0 ** -18, True, True, False),  # the smallest e above it
    ]


def boundary_table(W=208, rows=3):
    """pred, gt [1, rows, W]: the boundary pixels in row 1, everything else outside the mask (d = 0) -- every count and every sum of
    the table is known exactly.  W % 4 == 0."""
    gt = torch.zeros(1, rows, W)
    pred = torch.full((1, rows, W), 7.0)
    for x, d, p, *_ in boundary_rows():
        gt[0, 1, x], pred[0, 1, x] = d, p
    return pred, gt


# ------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lib_mod():
    import ecm_amd
    if not os.path.exists(ecm_amd._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm_amd._lib


def test_header_and_prototypes_declare_eval_kitti(lib_mod):
    for name in ("ecm_eval_kitti_scratch_bytes", "ecm_eval_kitti"):
        assert name in declared(), f"{name} is not declared in include/ecm_hip.h"
        assert name in lib_mod.PROTOTYPES
        assert hasattr(lib_mod.load(), name), f"libecm_hip.so does not export {name}"
    assert len(lib_mod.PROTOTYPES["ecm_eval_kitti"][1]) == 11
    assert lib_mod.query("ecm_abi_version") >= 6


def test_scratch_bytes_answers_without_a_gpu(lib_mod):
    for B, H, W in ((1, 1, 1), (2, 24, 40), (3, 1, 2049), (4, 384, 1248), (2, 1, KSPAN * KITTI_MAX_BLOCKS + 1), (33, 7, 9)):
        assert lib_mod.query("ecm_eval_kitti_scratch_bytes", B, H, W) == scratch_bytes(B, H, W), (B, H, W)
    assert lib_mod.query("ecm_eval_kitti_scratch_bytes", 4, 384, 1248) == 4 * 234 * 20 + 4 * 40
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert lib_mod.query("ecm_eval_kitti_scratch_bytes", *bad) == 0


def test_shape_contract_is_checked_before_the_gpu(lib_mod):
    lib, one = lib_mod.load(), 16            # non-null addresses that are never dereferenced: every call returns before a launch
    assert lib.ecm_eval_kitti(None, None, None, None, None, 0, 1, 1, 1, 192.0, None) == -1
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.ecm_eval_kitti(one, one, one, None, one, 1 << 20, B, H, W, 192.0, None) == -1        # ECM_EINVAL
    assert lib.ecm_eval_kitti(one, one, one, None, one, scratch_bytes(2, 24, 40) - 1, 2, 24, 40, 192.0, None) == -3   # ECM_ESCRATCH


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_reproduces_the_fixture(case):
    g = load_golden("g14_eval_kitti")
    pred, gt = g[case + ".pred"], g[case + ".gt"]
    want_loss, want_count = g[case + ".loss"].double().numpy(), g[case + ".count"].numpy()
    got = restate64(pred, gt)
    assert [int(v) for v in got[[4, 5, 6, 7]]] == [int(v) for v in want_count], "counts"
    if case == "empty":
        assert want_count.tolist() == [0, 0, 0, 0] and np.isnan(want_loss).all() and np.isnan(got[:4]).all()
        return
    assert want_count[0] > want_count[1] > 0 and want_count[3] < want_count[0]
    # loss_3: the reference forms it in fp32 from two exact integer sums; so does err3_fp32 -- the same bits
    assert got[3] == want_loss[3]
    # the means: the stored value is torch's fp32 mean.  Inputs lie on a grid of 1/4 (and a dozen boundary pixels), so its fp32
    # sum carries at most a few ulp and the division one rounding: within 4 ulp = 4 * 2^-23 relative of the fp64 mean
    for k in range(3):
        assert abs(got[k] - want_loss[k]) <= 4 * 2.0 ** -23 * abs(want_loss[k]), (COLUMNS[k], got[k], want_loss[k])
    # ... and the restated torch statements give the stored values themselves on this CPU
    assert torch.equal(torch_statements(pred, gt, "cpu").double(), torch.from_numpy(want_loss))


def test_fixture_sample_with_an_empty_mask():
    g = load_golden("g14_eval_kitti")
    pred, gt = g["sample_empty.pred"], g["sample_empty.gt"]
    assert np.isnan(restate64(pred[1:], gt[1:])[:4]).all() and restate64(pred[1:], gt[1:])[4:].tolist() == [0, 0, 0, 0]
    assert restate64(pred[:1], gt[:1]).tolist() == restate64(pred, gt).tolist()


def test_boundary_table_meets_each_boundary_exactly():
    pred, gt = boundary_table()
    e, mask, non, good = decisions(pred, gt)
    for x, d, p, in_mask, in_non, is_good in boundary_rows():
        d32, p32 = np.float32(d), np.float32(p)
        assert float(d32) == d and float(p32) == p, f"column {x}: d or p is not an fp32 number"
        assert float(np.float32(p32 - d32)) == p - d, f"column {x}: p - d is not exact in fp32"
        assert float(np.float32(np.float32(x) - d32)) == x - d, f"column {x}: x - d is not exact in fp32"
        assert (bool(mask[0, 1, x]), bool(non[0, 1, x]), bool(good[0, 1, x])) == (in_mask, in_non, is_good), f"column {x}"
        assert float(e[0, 1, x]) == abs(p - d)
    on = {r[0] for r in boundary_rows()}
    assert int(mask.sum()) == sum(r[3] for r in boundary_rows()) and len(on) == len(boundary_rows())
    # both neighbours of each threshold are present
    es = sorted(abs(p - d) for _, d, p, *_ in boundary_rows() if d == 1.0)
    assert es == [below(3.0), 3.0, above(3.0)]


def test_eval_kitti_refuses_cpu_tensors():
    import ecm_amd
    with pytest.raises(RuntimeError):
        ecm_amd.ops.eval_kitti(torch.zeros(1, 1, 4, 8), torch.zeros(1, 4, 8))
    with pytest.raises(RuntimeError):
        ecm_amd.ops.eval_epe(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), 4, 8, out=torch.zeros(6))
