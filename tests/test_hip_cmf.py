"""The `cmf` architecture on the MI355X (cmf/models/cmf.py): the super-resolution refinement decoder and the whole model
against the reference's own fp32 / fp64 runs (tests/golden/make_golden_cmf.py), the decoder's new kernels at production
geometry against PyTorch's convolutions, guard bands, determinism, the no-slow-path contract and a training step."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from oracle import ecm_oracle as O
from oracle.weights import seeded, tensor_for
from test_hip_fp64_yardstick import FLOOR, K, _check_params
from test_hip_guard_bands import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def _z(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _model(ecm, train=True):
    m = ecm.get_model("cmf")
    m.load_state_dict({k: tensor_for(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().train(train)


def _close(got, t64, e32, scale, what):
    """fp64 yardstick: |hip - fp64| within K x the reference-fp32's distance plus FLOOR x the quantity's scale."""
    e = float((got.detach().double().cpu() - torch.from_numpy(np.asarray(t64))).abs().max())
    assert e <= K * e32 + FLOOR * scale + 1e-12, f"{what}: max |hip - fp64| {e:.3e}, reference fp32 {e32:.3e}, scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------------ reference fixtures
def test_decoder_against_fp64_reference(ecm):
    """super_resolution_refinement alone (B = 2, 8x16 -> 32x64): output, the gradients of its four inputs and of every
    decoder parameter (norm, projection, and the full tensor where stored) vs the reference in fp64."""
    z = _z("g13_srr_decoder")
    srr = ecm.super_resolution_refinement(32, 2)
    srr.load_state_dict({k: tensor_for("srr." + k, v.shape) for k, v in srr.state_dict().items()})
    srr = srr.cuda()
    B, h, w = 2, 8, 16
    ins = dict(pred=seeded("g13.pred", B, h, w).abs() * 8.0, left=seeded("g13.left", B, 3, 4 * h, 4 * w),
               ref=seeded("g13.ref", B, 32, h, w), half=seeded("g13.half", B, 32, 2 * h, 2 * w))
    ins = {k: v.cuda().requires_grad_() for k, v in ins.items()}
    y = srr(ins["pred"].unsqueeze(0), ins["left"], ins["ref"], ins["half"])[0]
    (y * seeded("g13.G", *y.shape).cuda()).sum().backward()
    ecm.ops.check_async_errors()
    e32 = float(np.abs(z["y_32"].astype(np.float64) - z["y_64"]).max())
    _close(y, z["y_64"], e32, float(np.abs(z["y_64"]).max()), "decoder output")
    for k, t in ins.items():
        t64 = z[f"gin_{k}_64"]
        _close(t.grad, t64, float(np.abs(z[f"gin_{k}_32"].astype(np.float64) - t64).max()), float(np.abs(t64).max()), f"grad {k}")
    bad = []
    for k, p in srr.named_parameters():
        kk = "srr_" + k.replace(".", "_")
        g = p.grad.detach().double().cpu()
        n64, n32 = float(z["gn64_" + kk]), float(z["gn32_" + kk])
        p64, p32 = float(z["gp64_" + kk]), float(z["gp32_" + kk])
        if abs(float(g.norm()) - n64) > K * abs(n32 - n64) + FLOOR * n64 + 1e-12:
            bad.append(f"{k}: |g| {float(g.norm()):.6e} vs fp64 {n64:.6e} (reference fp32 {n32:.6e})")
        pj = float((g * seeded("proj:srr." + k, *g.shape).double()).sum())
        if abs(pj - p64) > K * abs(p32 - p64) + 2e-2 * n64 + 1e-12:
            bad.append(f"{k}: projection {pj:.6e} vs fp64 {p64:.6e} (reference fp32 {p32:.6e})")
        if "g64_" + kk in z:
            t64 = torch.from_numpy(z["g64_" + kk])
            e = (g - t64).abs()
            if float(e.max()) > K * float(z["e32max_" + kk]) + FLOOR * float(t64.abs().max()) + 1e-12:
                bad.append(f"{k}: max |hip - fp64| {float(e.max()):.3e} vs the reference fp32's {float(z['e32max_' + kk]):.3e}")
    assert not bad, "\n".join(bad)


def test_full_cmf_train_step_against_fp64_reference(ecm):
    """Whole cmf at 256x512: the three predictions, the training loss (train.py:162-181) and EVERY parameter's gradient vs the
    reference's fp64 run, with the reference-fp32's distance as the yardstick (test_hip_fp64_yardstick.py's rule)."""
    z = _z("g13_full_cmf_256x512_fp64")
    model = _model(ecm)
    left, right = seeded("g13.left_full", 1, 3, 256, 512).cuda(), seeded("g13.right_full", 1, 3, 256, 512).cuda()
    gt = (torch.rand(1, 256, 512, generator=torch.Generator().manual_seed(13)) * 191.0).cuda()
    o = model(left, right)
    assert all(tuple(p.shape) == (1, 1, 256, 512) for p in o)
    loss = O.train_loss(o, gt)
    loss.backward()
    ecm.ops.check_async_errors()
    for i in (1, 2, 3):
        d64 = (o[i - 1].detach().double().cpu()[..., ::4, ::4] - torch.from_numpy(z[f"o{i}_64"])).abs()
        r32 = (torch.from_numpy(z[f"o{i}_32"]).double() - torch.from_numpy(z[f"o{i}_64"])).abs()
        assert float(d64.max()) <= max(2e-3, K * float(r32.max())) and float(d64.mean()) <= max(1e-4 * i + 1e-4, K * float(r32.mean())), \
            (i, float(d64.max()), float(d64.mean()), float(r32.max()), float(r32.mean()))
    l64, l32 = float(z["loss_64"]), float(z["loss_32"])
    assert abs(float(loss.detach()) - l64) <= K * abs(l32 - l64) + 1e-5 * abs(l64), (float(loss.detach()), l64, l32)
    n_full, worst = _check_params(model, z, "cmf 256x512", population=True)
    assert n_full >= 10, n_full
    print("worst norm-error ratios vs the yardstick (cmf):", worst)


# ------------------------------------------------------------------------------------ new kernels at production geometry
def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("h,w", [(144, 240), (288, 480)])
def test_deconv2d_bias_production(ecm, h, w):
    """ConvTranspose2d(96 -> 64, 3, 2, 1, 1, bias) at B = 4 (both decoder stages): forward, data, weight and bias gradient
    against PyTorch's conv_transpose2d on the device."""
    g = torch.Generator(device="cuda").manual_seed(h)
    x = torch.randn(4, 96, h, w, device="cuda", generator=g).requires_grad_()
    wt = (torch.randn(96, 64, 3, 3, device="cuda", generator=g) * 0.05).requires_grad_()
    b = torch.randn(64, device="cuda", generator=g).requires_grad_()
    y = ecm.ops.deconv2d_k3s2_bias(x, wt, b)
    gy = torch.randn(y.shape, device="cuda", generator=g)
    gx, gw, gb = torch.autograd.grad(y, (x, wt, b), gy)
    ecm.ops.check_async_errors()
    xd, wd, bd = (t.detach().clone().requires_grad_() for t in (x, wt, b))
    yr = F.conv_transpose2d(xd, wd, bd, stride=2, padding=1, output_padding=1)
    rx, rw, rb = torch.autograd.grad(yr, (xd, wd, bd), gy)
    assert y.shape == yr.shape
    assert _rel(y, yr) < 1e-5 and _rel(gx, rx) < 1e-5, (_rel(y, yr), _rel(gx, rx))
    assert _rel(gw, rw) < 1e-4 and _rel(gb, rb) < 1e-4, (_rel(gw, rw), _rel(gb, rb))
    # the bias gradient against an fp64 sum
    assert _rel(gb.double(), gy.double().sum((0, 2, 3))) < 1e-5


def test_conv_out_production(ecm):
    """conv_out + ReLU, Conv2d(96 -> 1, 3x3, bias) at 576x960, B = 4: forward, data, weight and bias gradient against
    F.conv2d + relu on the device."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(4, 96, 576, 960, device="cuda", generator=g).requires_grad_()
    wt = (torch.randn(1, 96, 3, 3, device="cuda", generator=g) * 0.05).requires_grad_()
    b = torch.tensor([0.1], device="cuda").requires_grad_()
    y = ecm.ops.conv2d_c1_relu(x, wt, b)
    gy = torch.randn(y.shape, device="cuda", generator=g)
    gx, gw, gb = torch.autograd.grad(y, (x, wt, b), gy)
    ecm.ops.check_async_errors()
    xd, wd, bd = (t.detach().clone().requires_grad_() for t in (x, wt, b))
    yr = F.relu(F.conv2d(xd, wd, bd, padding=1))
    rx, rw, rb = torch.autograd.grad(yr, (xd, wd, bd), gy)
    assert y.shape == yr.shape
    # ReLU decisions of outputs within rounding of 0 may differ: compare where the two agree on the mask (all but a handful)
    agree = (y > 0) == (yr > 0)
    assert float(agree.float().mean()) > 0.9999
    assert _rel(y * agree, yr * agree) < 1e-5
    assert _rel(gx, rx) < 1e-3 and _rel(gw, rw) < 1e-3 and _rel(gb, rb) < 1e-3, (_rel(gx, rx), _rel(gw, rw), _rel(gb, rb))


def test_channel_sum(ecm):
    g = torch.Generator(device="cuda").manual_seed(3)
    for shape in [(4, 64, 576, 960), (3, 5, 7, 11), (1, 2, 1, 16385)]:
        x = torch.randn(shape, device="cuda", generator=g)
        got = ecm.ops.channel_sum(x)
        ref = x.double().sum((0, 2, 3))
        assert _rel(got.double(), ref) < 1e-5, shape


# ---------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("B,Ci,Co,h,w", [(1, 96, 64, 5, 7), (2, 8, 20, 9, 33), (1, 96, 64, 17, 70)])
def test_guard_bands_deconv2d_bias(ecm, B, Ci, Co, h, w):
    with guarded(ecm) as gd:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, Ci, h, w, device="cuda", generator=g).requires_grad_()
        wt = torch.randn(Ci, Co, 3, 3, device="cuda", generator=g).requires_grad_()
        b = torch.randn(Co, device="cuda", generator=g).requires_grad_()
        y = ecm.ops.deconv2d_k3s2_bias(x, wt, b)
        (y * torch.randn_like(y)).sum().backward()
        gd.check(f"deconv2d_bias {B}x{Ci}->{Co} {h}x{w}")


@pytest.mark.parametrize("B,Ci,H,W", [(1, 96, 37, 70), (2, 5, 33, 65), (1, 96, 130, 3), (3, 7, 1, 1)])
def test_guard_bands_conv_out(ecm, B, Ci, H, W):
    with guarded(ecm) as gd:
        g = torch.Generator(device="cuda").manual_seed(2)
        x = torch.randn(B, Ci, H, W, device="cuda", generator=g).requires_grad_()
        wt = torch.randn(1, Ci, 3, 3, device="cuda", generator=g).requires_grad_()
        b = torch.randn(1, device="cuda", generator=g).requires_grad_()
        y = ecm.ops.conv2d_c1_relu(x, wt, b)
        (y * torch.randn_like(y)).sum().backward()
        gd.check(f"conv_out {B}x{Ci} {H}x{W}")
        assert torch.isfinite(x.grad).all() and torch.isfinite(wt.grad).all()


def test_guard_bands_channel_sum(ecm):
    with guarded(ecm) as gd:
        ecm.ops.channel_sum(torch.randn(3, 5, 7, 11, device="cuda"))
        ecm.ops.channel_sum(torch.randn(2, 3, 16385, device="cuda"))
        gd.check("channel_sum")


# ------------------------------------------------------------------------------------------- model-level contracts
def test_backward_is_bit_reproducible(ecm):
    model = _model(ecm)
    left, right = seeded("det.left", 1, 3, 256, 512).cuda(), seeded("det.right", 1, 3, 256, 512).cuda()
    gt = (torch.rand(1, 256, 512, generator=torch.Generator().manual_seed(2)) * 191.0).cuda()
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        O.train_loss(model(left, right), gt).backward()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    bad = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not bad, f"gradients differ between two identical backward passes: {bad[:8]}"


@pytest.mark.parametrize("hw", [(576, 960), (384, 1248)])
def test_no_slow_path(ecm, hw):
    model = _model(ecm)
    ecm.models.SLOW_PATH_EVENTS.clear()
    left, right = seeded("sp.left", 1, 3, *hw).cuda(), seeded("sp.right", 1, 3, *hw).cuda()
    o = model(left, right)
    sum(p.mean() for p in o).backward()
    ecm.ops.check_async_errors()
    assert ecm.models.SLOW_PATH_EVENTS == [], ecm.models.SLOW_PATH_EVENTS
    assert all(tuple(p.shape) == (1, 1) + hw for p in o)


def test_training_step_576x960_b4(ecm):
    """One FlatBucketDDP + stereo_loss3 + Adam step (train.py:162-181) at 576x960, batch 4: finite loss and parameters."""
    from importlib import import_module
    D = import_module("explicit-context-mapping-for-stereo-matching_amd.dist")
    model = _model(ecm)
    ddp = D.FlatBucketDDP(model, 1)
    opt = torch.optim.Adam(ddp.params, lr=1e-3, betas=(0.9, 0.999))
    g = torch.Generator(device="cpu").manual_seed(7)
    left, right = torch.randn(4, 3, 576, 960, generator=g).cuda(), torch.randn(4, 3, 576, 960, generator=g).cuda()
    gt = (torch.rand(4, 576, 960, generator=g) * 191.0).cuda()
    ddp.zero_grad()
    preds = model(left, right)
    loss, _ = ecm.ops.stereo_loss3(preds, gt, 192)
    loss.backward()
    ddp.allreduce_gradients()
    opt.step()
    torch.cuda.synchronize()
    ecm.ops.check_async_errors()
    assert torch.isfinite(loss).all()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
