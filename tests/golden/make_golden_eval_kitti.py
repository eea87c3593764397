#!/usr/bin/env python3
"""Golden fixture g14 for the KITTI validation leg: eval_kitti.py:84-103, the three masks with d > 0, the
masked mean errors of output3 on the whole frame and the 3-px / 5 % error rate of a batch.

Those statements sit inside a script's loop over checkpoints and a data loader, so they cannot be imported or called: they are
EXECUTED, read from /root/reference at generation time -- nothing is copied into the repo, only inputs and outputs are stored.
Build container only.  Usage: python -B tests/golden/make_golden_eval_kitti.py

Inputs: ground truth and prediction from oracle.weights.seeded on a grid of 1/4 px (compresses well; every sum is exact), and in
sample 0 of every case a hand-placed row that meets each decision of the statements: d == 0, d < 0, d == maxdisp and its fp32
neighbour below, x - d == 0 and one ulp past it, |e| == 3 and both fp32 neighbours, |e| on either side of 0.05 * d.
Cases: b2, b1, empty (no pixel under the mask: NaN), sample_empty (sample 1 has an empty mask, the batch has not)."""
from __future__ import annotations

import os
import sys
import textwrap
import time

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from oracle.weights import seeded  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self          # eval_kitti.py calls .cuda(2) on everything
REF = "/root/reference/eval_kitti.py"
H, W = 24, 40


def run_reference_lines(path, first, last, ns):
    """exec lines first..last (1-based, inclusive) of a reference file in namespace `ns`, dedented."""
    lines = open(path).read().split("\n")[first - 1:last]
    exec(compile(textwrap.dedent("\n".join(lines)), f"{path}:{first}-{last}", "exec"), ns)
    return ns


def boundary_row(gt, pred):
    """Row 0 of sample 0: (column, d, e = pred - d), every difference exact in fp32."""
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(-1e9)))
    above = lambda v: float(np.nextafter(np.float32(v), np.float32(1e9)))
    rows = [(0, 0.0, 1.0), (1, -1.0, 1.0), (2, 192.0, 1.0), (3, below(192.0), -1.0),      # mask edges
            (4, 4.0, 0.5), (5, above(5.0), 0.5), (30, 30.0, -0.5),                        # x - d == 0 / one ulp past it
            (6, 1.0, 3.0), (7, 1.0, below(3.0)), (8, 1.0, -above(3.0)),                   # |e| against 3 (0.05 d = 0.05)
            (9, 100.0, 4.0), (10, 100.0, -6.0), (11, 64.0, 3.125), (12, 64.0, 3.25)]      # |e| >= 3 against 0.05 d (5; 3.2)
    for x, d, e in rows:
        gt[0, 0, x] = d
        pred[0, 0, x] = float(np.float32(d) + np.float32(e))
        assert float(pred[0, 0, x]) - float(gt[0, 0, x]) == float(np.float32(e)), (x, d, e)


def case(name, B, empty=()):
    gt = torch.round(seeded(f"g14.{name}.gt", B, H, W).abs() * 25.0 * 4.0) / 4.0          # about half with x - d >= 0
    gt[:, ::4, ::9] += 150.0                                                              # some beyond 192
    gt[:, ::5, ::7] = 0.0
    pred = gt + torch.round(seeded(f"g14.{name}.e", B, H, W) * 2.5 * 4.0) / 4.0
    boundary_row(gt, pred)
    outside = torch.tensor([0.0, 192.0, 200.0, -1.0]).repeat(H * W // 4).view(H, W)
    for b in empty:
        gt[b] = outside
    return pred.unsqueeze(1), gt


out = {}
for name, B, empty in (("b2", 2, ()), ("b1", 1, ()), ("empty", 2, (0, 1)), ("sample_empty", 2, (1,))):
    pred, gt = case(name, B, empty)
    ns = dict(torch=torch, time=time, np=np, left=torch.zeros(1), right=torch.zeros(1), disparity=gt.clone(),
              model=lambda l, r: (pred * 0.5, pred * 0.7, pred))
    run_reference_lines(REF, 76, 77, ns)                  # ones, zeros
    run_reference_lines(REF, 84, 90, ns)                  # local, the three masks
    run_reference_lines(REF, 93, 93, ns)                  # the model call
    run_reference_lines(REF, 96, 103, ns)                 # squeeze, the three means, error_map, total, loss_3
    out[name + ".pred"] = pred.numpy()
    out[name + ".gt"] = gt.numpy()
    out[name + ".loss"] = np.array([ns[k].item() for k in ("loss", "loss_non", "loss_true", "loss_3")], dtype=np.float32)
    out[name + ".count"] = np.array([int(ns["mask"].sum()), int(ns["mask_non"].sum()), int(ns["mask_true"].sum()),
                                     int(ns["error_map"].sum())], dtype=np.int64)
    print(name, out[name + ".loss"], out[name + ".count"])

path = os.path.join(ROOT, "tests", "golden", "g14_eval_kitti.npz")
np.savez_compressed(path, **out)
print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
