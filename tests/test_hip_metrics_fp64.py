"""The kernels that close a training step and the evaluation leg -- stereo_loss3 with its backward (csrc/loss.hip), the three-mask
EPE and the uint16 KITTI image (csrc/eval.hip), the KITTI padding of frame_prep -- on their decision boundaries and around the edges
of their reduction grids, reached through ecm_amd.ops.

Operands.  `loss_table` / `epe_table` of tests/test_costvol_geometry.py: values on a dyadic grid, every boundary met exactly
(gt == 0, gt == maxdisp, |p - gt| == 1 and 1 -+ 2^-10, |p3 - gt| == 3 and its fp32 neighbour, |p3 - gt| on either side of
0.05f * gt; d == 0, d < 0, d == maxdisp, x - d == 0 against one ulp below), with every fp32 difference exact (shown on the CPU
there).  Sizes: fewer elements than one workgroup, 64 partials against 65 (stereo_loss_final strides its lanes by 64), exactly the
cap of 1024 workgroups and past it, where a thread walks more than 8 elements.

Checks.
  * Discrete results -- the mask count and the numerator of err3; the three counts of the EPE -- equal the oracle's fp32 statements
    (O.train_loss / O.kitti_metrics / O.sceneflow_eval_epe, the reference program's arithmetic) exactly.  err3 itself is then
    float(100 - good / count * 100) in double, as the kernel forms it: compared exactly too.
  * Continuous results -- the loss, the three means, the EPE, the three gradient maps under a non-unit upstream gradient; the three
    EPE means -- against the fp64 sum over that same mask under the yardstick of the fp64 suites:
    |hip - q64| <= K * e32 + FLOOR * max|q64| with e32 the larger error of torch fp32 on the CPU and on the device.  Each check prints
    `CVRATIO <path> <quantity> <ratio>` (DESIGN.md section 4 holds the worst as measured on the MI355X).
  * Gradients outside the mask are exactly zero; an empty mask gives NaN forward and what the oracle's autograd gives backward.
  * Every case runs twice on fresh operands and must repeat bit for bit; the allocator's free blocks hold NaN before each run."""
import warnings

import numpy as np
import pytest
import torch

import oracle.ecm_oracle as O
import test_costvol_geometry as G
from test_hip_conv3d_fp64 import DEV, FLOOR, K
from test_hip_costvol_fp64 import poison

pytestmark = pytest.mark.gpu

GUP = 1.5                      # upstream gradient on the loss
WEIGHTS = (0.5, 0.7, 1.0)


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def yardstick(path, name, what, got, ref, draws, fails):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    each = [float((torch.as_tensor(d).detach().cpu().double() - ref).abs().max()) for d in draws]
    e32, scale = max(each), float(ref.abs().max())
    err = float((got.detach().cpu().double() - ref).abs().max())
    bound = K * e32 + FLOOR * scale
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"CVRATIO {path} {what} {ratio:.3f}   # {name}: err {err:.3e}, e32 {e32:.3e} [{each[0]:.2e} {each[1]:.2e}], max|ref| {scale:.3e}")
    if not err <= bound:
        fails.append(f"{name}: {what} on {path}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")


def torch_loss(gt, ps, device):
    """The oracle's fp32 statements on `device`: {loss, m1..m3, epe, err3, count, g1..g3}."""
    gt = gt.to(device)
    ps = [p.to(device).clone().requires_grad_() for p in ps]
    mask = (gt < G.MAXDISP) & (gt > 0)
    loss = O.train_loss([p.view(1, 1, -1) for p in ps], gt.view(1, -1))
    (loss * GUP).backward()
    epe, err3 = O.kitti_metrics(ps[2].detach(), gt)
    out = {"loss": loss.detach(), "epe": epe, "err3": err3, "count": int(mask.sum())}
    for k, p in enumerate(ps):
        out["m%d" % (k + 1)] = torch.nn.functional.smooth_l1_loss(p.detach()[mask], gt[mask], reduction="mean")
        out["g%d" % (k + 1)] = p.grad
    return out


def hip_loss(ecm, gt, ps):
    poison()
    g = gt.to(DEV)
    pd = [p.to(DEV).view(1, 1, -1).requires_grad_() for p in ps]
    loss, met = ecm.ops.stereo_loss3(pd, g.view(1, -1), G.MAXDISP, WEIGHTS)
    (loss * GUP).backward()
    return {"loss": loss.detach(), "met": met.detach().clone(), **{"g%d" % (k + 1): p.grad.view(-1) for k, p in enumerate(pd)}}


@pytest.mark.parametrize("name", sorted(G.LOSS, key=lambda k: G.LOSS[k].n))
def test_stereo_loss3_fp64(ecm, name):
    n = G.LOSS[name].n
    gt, p1, p2, p3 = G.loss_table(n)
    ps = (p1, p2, p3)
    ref, mask = G.loss_reference(gt, ps, GUP, G.MAXDISP, WEIGHTS)
    a, b = hip_loss(ecm, gt, ps), hip_loss(ecm, gt, ps)
    cpu, dev = torch_loss(gt, ps, "cpu"), torch_loss(gt, ps, DEV)
    fails = []
    path = "loss.%dwg" % G.reduce_blocks(n)
    for k in a:
        if not torch.equal(a[k], b[k]):
            fails.append(f"{name}: {k} differs between two runs")
    met = a["met"].cpu()
    # discrete: the count and the numerator of err3 are the oracle's, exactly
    assert cpu["count"] == ref["count"] == dev["count"] and ref["count"] > 0
    good_oracle = round((100.0 - float(cpu["err3"])) * ref["count"] / 100.0)
    print(f"CVCOUNT {path} count {int(met[1])} / {ref['count']}  good {ref['good']} (oracle fp32: {good_oracle})   # {name}")
    assert good_oracle == ref["good"], "the fp32 statements of the oracle and their restatement disagree"
    if float(met[1]) != float(ref["count"]):
        fails.append(f"{name}: mask count {float(met[1])} != {ref['count']}")
    err3_want = torch.tensor(100.0 - ref["good"] / ref["count"] * 100.0, dtype=torch.float64).float()
    if float(met[3]) != float(err3_want) or round((100.0 - float(met[3])) * ref["count"] / 100.0) != ref["good"]:
        fails.append(f"{name}: err3 {float(met[3])!r} is not that of {ref['good']} good pixels of {ref['count']} ({float(err3_want)!r})")
    if float(met[0]) != float(a["loss"]) or float(met[7]) != 0.0:
        fails.append(f"{name}: metrics[0] is not the loss / metrics[7] is not 0")
    # continuous
    yardstick(path, name, "loss", a["loss"], ref["loss"], [cpu["loss"], dev["loss"]], fails)
    for k, slot in (("m1", 4), ("m2", 5), ("m3", 6), ("epe", 2)):
        yardstick(path, name, k, met[slot], ref[k], [cpu[k], dev[k]], fails)
    for k in ("g1", "g2", "g3"):
        yardstick(path, name, k, a[k], ref[k], [cpu[k], dev[k]], fails)
        if not bool((a[k].cpu()[~mask] == 0).all()):
            fails.append(f"{name}: {k} is not exactly zero outside the mask")
    ecm.ops.check_async_errors()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [255, 2049])
def test_stereo_loss3_empty_mask(ecm, n):
    """Nothing inside the mask (gt of 0, maxdisp and beyond): NaN forward, and backward what the oracle's autograd gives."""
    _, p1, p2, p3 = G.loss_table(n)
    gt = torch.tensor([0.0, 192.0, 200.0, -1.0]).repeat(n // 4 + 1)[:n]
    want = torch_loss(gt, (p1, p2, p3), "cpu")
    got = hip_loss(ecm, gt, (p1, p2, p3))
    assert torch.isnan(want["loss"]) and torch.isnan(got["loss"]) and float(got["met"][1]) == 0.0
    assert torch.isnan(got["met"][[0, 2, 3, 4, 5, 6]]).all()
    for k in ("g1", "g2", "g3"):
        assert torch.equal(got[k].cpu(), want[k]), k
        assert bool((want[k] == 0).all())


def hip_epe(ecm, pred, gt, c):
    poison()
    return ecm.ops.eval_epe(pred.to(DEV), gt.to(DEV), c.ch, c.cw, G.MAXDISP).clone()


@pytest.mark.parametrize("name", sorted(G.EPE))
def test_eval_epe_fp64(ecm, name):
    c = G.EPE[name]
    pred, gt = G.epe_table(c)
    means, counts, err, masks = G.epe_reference(pred, gt, c.ch, c.cw)
    a, b = hip_epe(ecm, pred, gt, c), hip_epe(ecm, pred, gt.unsqueeze(1).squeeze(1), c)
    fails = []
    if not torch.equal(a, b):
        fails.append(f"{name}: two runs differ")
    got = a.cpu()
    path = "epe.%dwg" % G.reduce_blocks(c.B * c.ch * c.cw)
    print(f"CVCOUNT {path} counts {[int(v) for v in got[3:]]} / {counts}   # {name}")
    if [float(v) for v in got[3:]] != [float(v) for v in counts]:
        fails.append(f"{name}: counts {[float(v) for v in got[3:]]} != {counts}")
    err_dev = err.to(DEV)
    for k, what in enumerate(("epe", "epe_non", "epe_true")):
        if counts[k] == 0:
            if not torch.isnan(got[k]):
                fails.append(f"{name}: {what} over an empty mask is {float(got[k])}, not NaN")
            continue
        draws = [torch.mean(err[masks[k]]), torch.mean(err_dev[masks[k].to(DEV)])]
        yardstick(path, name, what, got[k], means[k], draws, fails)
    ecm.ops.check_async_errors()
    assert not fails, "\n".join(fails)


def test_disparity_to_uint16_past_one_launch(ecm):
    """33 samples of ragged sizes (a launch carries 32): values * 256 in [0, 65535.996], exact integers and the largest fp32 below
    an integer among them, against O.kitti_disparity_uint16 per sample; bytes outside a sample's h x w are zero."""
    B, Hp, Wp = G.U16["B"], G.U16["Hp"], G.U16["Wp"]
    assert B > G.CHUNK
    g = torch.Generator().manual_seed(33)
    ks = torch.randint(0, 65536, (B, Hp, Wp), generator=g).float()
    below = torch.nextafter(ks + 1, torch.zeros(()))                       # the largest fp32 below k + 1: truncates to k
    frac = ks + torch.rand(B, Hp, Wp, generator=g) * 0.996
    pick = torch.arange(B * Hp * Wp).view(B, Hp, Wp) % 3
    v = torch.where(pick == 0, ks, torch.where(pick == 1, below, frac))
    v[0, -1, -1], v[32, -1, -1], v[31, -1, -2], v[32, -1, -2] = 0.0, 65535.996, 65535.0, 1.0 - 2.0 ** -24
    assert float(v.min()) >= 0 and float(v.max()) == 65535.99609375
    pred = v / 256.0                                                       # exact: a power of two
    assert torch.equal(pred * 256.0, v)
    hs = [1 + (5 * b) % Hp for b in range(B)]
    ws = [1 + (7 * b) % Wp for b in range(B)]
    hs[32], ws[32], hs[0], ws[0] = Hp, Wp, Hp, Wp
    poison()
    img = ecm.ops.disparity_to_uint16(pred.to(DEV), hs, ws).cpu().numpy()
    assert img.dtype == np.uint16 and img.shape == (B, max(hs), max(ws))
    for b in range(B):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = O.kitti_disparity_uint16(pred[b:b + 1], hs[b], ws[b])
        assert np.array_equal(img[b, :hs[b], :ws[b]], want), b
        assert not img[b, hs[b]:].any() and not img[b, :, ws[b]:].any(), b
    assert img[32, Hp - 1, Wp - 1] == 65535 and img[32, Hp - 1, Wp - 2] == 0 and img[0, Hp - 1, Wp - 1] == 0


@pytest.mark.parametrize("form", ["float32", "packed_fp32", "packed_fp16"])
def test_frame_prep_kitti_eval_past_one_launch(ecm, form):
    """33 frames of 5 x 7 padded to 8 x 12 (a launch carries 32): samples 0, 31 and 32 bit-exact against O.kitti_eval_sample."""
    k = G.KITTI_PREP
    B, H, W, th, tw = k["B"], k["H"], k["W"], k["th"], k["tw"]
    assert B > G.CHUNK
    rs = np.random.RandomState(12)
    rgb = rs.randint(0, 256, size=(B, H, W, 6)).astype(np.uint8)
    disp = (rs.randint(0, 2048, size=(B, H, W)) / 8.0).astype(np.float32)            # multiples of 1/8 below 256: exact in fp16
    frames = np.concatenate([rgb.astype(np.float32), disp[..., None]], 3)
    if form == "float32":
        src = torch.from_numpy(frames).to(DEV)
    else:
        d = torch.from_numpy(disp).to(DEV)
        src = (torch.from_numpy(rgb).to(DEV), d.half() if form == "packed_fp16" else d)
        assert torch.equal(d.half().float(), d)
    poison()
    left, right, dsp, image = ecm.ops.frame_prep_kitti_eval(src, th, tw, want_image=True)
    assert left.shape == (B, 3, th, tw) and dsp.shape == (B, th, tw)
    for b in (0, 31, 32):
        l, r, d = O.kitti_eval_sample(frames[b], th, tw)
        assert torch.equal(left[b].cpu(), l) and torch.equal(right[b].cpu(), r) and torch.equal(dsp[b].cpu(), d), b
        pad = O.kitti_eval_pad(np.array(frames[b], copy=True), th, tw)
        assert np.array_equal(image[b].cpu().numpy().transpose(1, 2, 0), pad[..., :3]), b
    ecm.ops.check_async_errors()
