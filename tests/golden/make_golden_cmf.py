#!/usr/bin/env python3
"""Golden fixtures of the `cmf` architecture (cmf/models/cmf.py: the stride-2-stem encoder, the cmfsm hourglass stack and the
super-resolution refinement decoder), produced by the REFERENCE's own code, in fp32 and in fp64 (the recipe of
make_golden_fp64.py), on seeded inputs and per-key weights (oracle.weights.tensor_for) -- the fixtures hold no weights:

  cmf_state_shapes.json           state_dict key -> shape of get_model("cmf")
  g13_srr_decoder.npz             super_resolution_refinement(32, 2) alone (cmf.py:227-264), B = 2, 8x16 -> 32x64: forward
                                  output, every `srr.*` parameter's gradient and the gradients of its four inputs
  g13_full_cmf_256x512_fp64.npz   the whole cmf at 256x512: the three predictions (sub-sampled), the smooth-L1 training loss
                                  (train.py:162-181) and every parameter's gradient as norm + seeded projection (fp32 and
                                  fp64) plus the full tensors of a dozen parameters -- the form test_hip_fp64_yardstick.py reads

Build container only (needs the reference tree).  Usage: python -B tests/golden/make_golden_cmf.py [shapes] [srr] [full]"""
from __future__ import annotations

import json
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

for name in ("torchvision", "torchvision.models", "cmf.caffe_pb2"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.path.insert(0, "/root/reference")
from cmf.models import get_model  # noqa: E402
from cmf.models.cmf import super_resolution_refinement  # noqa: E402
from oracle.weights import seeded, tensor_for  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)
_F32 = torch.FloatTensor

# decoder fixture geometry: batch, low-res (1/4) map, full-res image
SRR_B, SRR_h, SRR_w = 2, 8, 16
FULL_HW = (256, 512)
# full gradient tensors stored next to every parameter's norm + projection (the larger kernels -- conv2, the two deconvs,
# dres0 -- have norm + projection only: the fixtures stay under 1 MiB)
FULL_GRADS = ("srr.conv1.0.0.weight", "srr.deconv_module_list.0.0.bias", "srr.deconv_module_list.1.0.bias",
              "srr.deconv_module_list.1.1.weight", "srr.rgb_fea.0.0.weight", "srr.conv2.1.weight", "srr.conv_out.weight",
              "srr.conv_out.bias", "classif1.2.weight", "feature_extraction.firstconv.0.0.weight",
              "feature_extraction.lastconv.2.weight")
SRR_FULL_MAX = 20000          # decoder fixture: full tensors of the parameters up to this size, norm + projection of all


def set_precision(double):
    torch.FloatTensor = torch.DoubleTensor if double else _F32          # the reference allocates the cost volume with it


def squeeze_fp32(out):
    """Replace the reference-fp32 full gradient tensors by their distance from the fp64 truth (max-abs and rms): the yardstick."""
    for k in [k for k in out if k.startswith("g32_")]:
        e = out[k].astype(np.float64) - out["g64_" + k[4:]]
        out["e32max_" + k[4:]] = np.abs(e).max()
        out["e32rms_" + k[4:]] = np.sqrt((e ** 2).mean())
        del out[k]


def srr_inputs():
    """The decoder fixture's inputs (the GPU test rebuilds them from the same names)."""
    B, h, w = SRR_B, SRR_h, SRR_w
    return dict(pred=seeded("g13.pred", B, h, w).abs() * 8.0, left=seeded("g13.left", B, 3, 4 * h, 4 * w),
                ref=seeded("g13.ref", B, 32, h, w), half=seeded("g13.half", B, 32, 2 * h, 2 * w))


def make_shapes():
    sd = get_model("cmf").state_dict()
    with open(os.path.join(OUT, "cmf_state_shapes.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sd.items()}, f)
    print("cmf_state_shapes.json:", len(sd), "tensors", flush=True)


def make_srr():
    out = {}
    for double in (False, True):
        tag = "64" if double else "32"
        m = super_resolution_refinement(32, 2)
        m.load_state_dict({k: tensor_for("srr." + k, v.shape) for k, v in m.state_dict().items()})
        ins = srr_inputs()
        if double:
            m = m.double()
            ins = {k: v.double() for k, v in ins.items()}
        ins = {k: v.requires_grad_() for k, v in ins.items()}
        y = m(ins["pred"], ins["left"], ins["ref"], ins["half"])
        G = seeded("g13.G", *y.shape)
        (y * (G.double() if double else G)).sum().backward()
        out[f"y_{tag}"] = y.detach().numpy()
        for k, v in ins.items():
            out[f"gin_{k}_{tag}"] = v.grad.numpy()
        for k, p in m.named_parameters():
            kk = "srr_" + k.replace(".", "_")
            g = p.grad.detach().double()
            out[f"gn{tag}_{kk}"] = g.norm().numpy()
            out[f"gp{tag}_{kk}"] = (g * seeded("proj:srr." + k, *g.shape).double()).sum().numpy()
            if p.numel() <= SRR_FULL_MAX:
                out[f"g{tag}_{kk}"] = g.numpy() if double else g.float().numpy()
        print("srr", tag, tuple(y.shape), float(y.detach().abs().mean()), flush=True)
    squeeze_fp32(out)
    np.savez_compressed(os.path.join(OUT, "g13_srr_decoder.npz"), **out)
    print("wrote g13_srr_decoder", os.path.getsize(os.path.join(OUT, "g13_srr_decoder.npz")) // 1024, "KiB", flush=True)


def run_full(double):
    set_precision(double)
    model = get_model("cmf")
    model.load_state_dict({k: tensor_for(k, v.shape) for k, v in model.state_dict().items()})
    H, W = FULL_HW
    left, right = seeded("g13.left_full", 1, 3, H, W), seeded("g13.right_full", 1, 3, H, W)
    gt = torch.rand(1, H, W, generator=torch.Generator().manual_seed(13)) * 191.0
    if double:
        model, left, right, gt = model.double(), left.double(), right.double(), gt.double()
    model.train()
    o1, o2, o3 = model(left, right)
    mask = (gt < 192) & (gt > 0)
    s1, s2, s3 = o1.squeeze(1), o2.squeeze(1), o3.squeeze(1)
    loss = (0.5 * F.smooth_l1_loss(s1[mask], gt[mask], reduction="mean")
            + 0.7 * F.smooth_l1_loss(s2[mask], gt[mask], reduction="mean")
            + F.smooth_l1_loss(s3[mask], gt[mask], reduction="mean"))
    loss.backward()
    return model, (o1, o2, o3), loss


def make_full():
    out = {}
    for double in (False, True):
        tag = "64" if double else "32"
        model, preds, loss = run_full(double)
        for i, p in enumerate(preds, 1):
            out[f"o{i}_{tag}"] = p.detach()[..., ::4, ::4].contiguous().numpy()
        out[f"loss_{tag}"] = loss.detach().numpy()
        for k, p in model.named_parameters():
            kk = k.replace(".", "_")
            g = p.grad.detach().double()
            out[f"gn{tag}_{kk}"] = g.norm().numpy()
            out[f"gp{tag}_{kk}"] = (g * seeded("proj:" + k, *g.shape).double()).sum().numpy()
            if k in FULL_GRADS:
                out[f"g{tag}_{kk}"] = g.numpy() if double else g.float().numpy()
        print("full cmf", tag, "loss", float(loss), flush=True)
    set_precision(False)
    squeeze_fp32(out)
    path = os.path.join(OUT, "g13_full_cmf_256x512_fp64.npz")
    np.savez_compressed(path, **out)
    print("wrote g13_full_cmf_256x512_fp64", os.path.getsize(path) // 1024, "KiB", flush=True)


if __name__ == "__main__":
    todo = sys.argv[1:] or ["shapes", "srr", "full"]
    for what in todo:
        {"shapes": make_shapes, "srr": make_srr, "full": make_full}[what]()
