"""The table of tests/test_hip_forward_contract.py (on the MI355X) and tests/test_forward_contract_cpu.py (anywhere): one row per
forward-only op of ops.py -- every function under @torch.no_grad() there, plus eval_epe, eval_kitti and disparity_to_uint16 --
and the builders of the operand variants the contract is stated in.

ROWS[op] = Row(cases, operands, roles, call, restatement, rule, hold, batch, sequential, inplace, exempt, masks):
  cases        the names of the row's shapes; operands(case) builds them on the CPU
  operands     case -> an ordered dict of everything `call` needs: CPU tensors and plain parameters
  roles        operand name -> role, for the operands that are DEVICE tensors: "plane" (fp32 or int32 [B,H,W] / [B,1,H,W]),
               "mask" (bool or uint8), "guide" (guide or attribute planes [B,C,H,W]), "head" (a head volume or its weights),
               "image" (a raw frame), "volume" (a plane of a TSDF volume, used in place or read)
  call         (ops, operands on the device) -> the tuple of output tensors
  restatement  "module:function" of the fp64 or exact restatement that the op's own test file holds
  rule         that file's rule for it, in words
  hold         (ops, CPU operands, CPU outputs, device operands, device outputs) -> asserts the rule on the clean result, with
               the op file's own check helper where it has one
  batch        per output, the dim along which the per-image results stack; None for a batch-wide output (exempt, reason in
               `exempt["batch:<index>"]`)
  matrices     the names of the per-image matrices, sliced per image beside the tensors
  sequential   the op's "batch" is a sequence of in-place updates (volume_integrate's views)
  inplace      the operands the op is allowed to change
  exempt       variant -> reason, for every variant the row does not run
  masks        mask operand name -> True where the op's header states the rule as `valid != 0` (uint8 0/2/255 is run)"""
import collections

import torch

from oracle.weights import seeded

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
B = 3
SIZES = {"odd": (37, 61), "w4": (40, 64)}
VOLUMES = {"4x4x64": (4, 4, 64), "5x5x17": (5, 5, 17)}
VARIANTS = ("strided", "misaligned", "mask_forms", "side_stream", "batch", "untouched", "recycled", "twice")

Row = collections.namedtuple("Row", "cases operands roles call restatement rule hold batch matrices sequential inplace exempt masks")
ROWS = {}


def _row(name, cases, operands, roles, call, restatement, rule, hold=None, batch=(0,), matrices=(), sequential=False, inplace=(),
         exempt=None, masks=None):
    assert name not in ROWS, name
    ROWS[name] = Row(tuple(cases), operands, dict(roles), call, restatement, rule, hold, tuple(batch), tuple(matrices), sequential,
                     tuple(inplace), dict(exempt or {}), dict(masks or {}))


# ---- the variant builders: they run on CPU tensors as on device tensors ----------------------------------------------------------------
def poison_of(t):
    """What a slack element holds: NaN in a float plane, 255 in a mask or a raw frame, -1 in an integer plane."""
    return NAN if t.is_floating_point() else (True if t.dtype == torch.bool else (255 if t.dtype == torch.uint8 else -1))


def strided(t):
    """(view, buffer): t's values as columns 1 : W+1 of a buffer W + 3 wide whose slack columns hold poison."""
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), poison_of(t), dtype=t.dtype, device=t.device)
    view = buf[..., 1:t.shape[-1] + 1]
    view.copy_(t)
    return view, buf


def slack_intact(t, buf):
    """The slack columns of strided()'s buffer still hold their poison."""
    W = t.shape[-1]
    slack = torch.cat([buf[..., :1], buf[..., W + 1:]], -1)
    if t.is_floating_point():
        return bool(torch.isnan(slack).all())
    return bool((slack == poison_of(t)).all())


def off_by_one(t):
    """t's values, contiguous, at an address 4 bytes past a 16-byte boundary (4-byte elements), as off_by_one of
    tests/test_hip_sparsification.py builds them."""
    assert t.element_size() == 4
    raw = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    at = (1 - raw.data_ptr() // 4) % 4
    out = raw[at:at + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def odd_byte(t):
    """A one-byte plane (bool, uint8) at an address that is 1 past a multiple of 4."""
    assert t.element_size() == 1
    raw = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    at = (1 - raw.data_ptr()) % 4
    out = raw[at:at + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def misaligned(t):
    return odd_byte(t) if t.element_size() == 1 else off_by_one(t)


def expanded(t, dim=0):
    """(stride-0 batch, its contiguous twin): image 0 of t, B times along `dim`."""
    one = t.narrow(dim, 0, 1)
    shape = list(t.shape)
    view = one.expand(shape)
    return view, view.contiguous()


def four_dim(t):
    """The other form of a plane: [B,H,W] as [B,1,H,W], and [B,1,H,W] as [B,H,W]."""
    return t.unsqueeze(1) if t.dim() == 3 else t[:, 0]


def mask_forms(m, nonzero_rule):
    """The forms of a bool mask that must decide alike: uint8 of 0/1 and, where the rule is `valid != 0`, uint8 of 0, 2 and 255."""
    forms = {"uint8 0/1": m.to(torch.uint8)}
    if nonzero_rule:
        idx = torch.arange(m.numel(), device=m.device).view(m.shape)
        forms["uint8 0/2/255"] = torch.where(m, torch.where(idx % 2 == 0, 2, 255), 0).to(torch.uint8)
    return forms


def bits_equal(a, b):
    """Bit for bit: fp32 as int32 (NaN meets NaN of the same bits), every other dtype by its own integer view."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---- operands --------------------------------------------------------------------------------------------------------------------------
def _rigid(*a):
    from test_disp_warp_cpu import rigid
    return rigid(*a)


POSES = lambda: torch.stack([_rigid(0.004, 0.011, -0.002, 0.04, -0.015, 0.05), torch.eye(4, dtype=F64),     # noqa: E731
                             _rigid(-0.01, 0.02, 0.0, -0.06, 0.03, -0.04)])


def scene(case, dirty=True):
    """B views of the three-plane scene of tests/test_motion_align_cpu.py at the case's size, with noise and, where dirty, a few
    NaN, inf, zero and negative pixels; (disp [B,H,W] fp32, Q)."""
    from test_motion_align_cpu import PLANES, render, scene_q
    H, W = SIZES[case]
    Q = scene_q(H, W)
    d = torch.stack([render(p, H, W, PLANES, Q) for p in POSES()]).to(F32) + 0.01 * seeded(f"fc.scene.{case}", B, H, W)
    if dirty:
        r = torch.rand(B, H, W, generator=torch.Generator().manual_seed(H))
        for k, bad in enumerate((NAN, float("inf"), 0.0, -2.0)):
            d[(r >= 0.004 * k) & (r < 0.004 * (k + 1))] = bad
    return d, Q


def valid_mask(name, shape, share=0.1):
    return torch.rand(shape, generator=torch.Generator().manual_seed(sum(map(ord, name)))) >= share


def _plane_case(name, case, scale=3.0, offset=8.0):
    H, W = SIZES[case]
    return seeded(f"fc.{name}.{case}", B, H, W) * scale + offset


def box(dims):
    """(origin, voxel) of a grid of dims = (nz, ny, nx) centred 3 m in front of the first camera, 1.6 m along its longest side
    (the box of tests/test_hip_disp_volume.py)."""
    nz, ny, nx = dims
    voxel = 1.6 / max(max(dims) - 1, 1)
    return (-voxel * (nx - 1) / 2, -voxel * (ny - 1) / 2, 3.0 - voxel * (nz - 1) / 2), voxel


TRUNC = 0.25


# heads: c [NH,B,D,h,w] with D <= 12; the full-resolution maps are h*scale x w*scale
def _head_c(name, D, h, w):
    return seeded(f"fc.{name}.c", 2, B, D, h, w)


def _eight(case):
    h, w = {"odd": (9, 15), "w4": (10, 16)}[case]
    return collections.OrderedDict(c=_head_c("eight." + case, 6, h, w), w9=torch.softmax(seeded(f"fc.eight.w9.{case}", B, 9, 4 * h, 4 * w), 1),
                                   scale=4, radius=4)


def _volume_head(case):
    h, w = {"odd": (5, 7), "w4": (5, 8)}[case]
    return collections.OrderedDict(c=_head_c("vm." + case, 6, h, w), m5=seeded(f"fc.vm.m5.{case}", B, 5, 8 * h, 8 * w, scale=0.5),
                                   mt3=seeded(f"fc.vm.mt3.{case}", B, 3, 8 * h, 8 * w, scale=0.5), scale=8, radius=2)


def _trilinear(case):
    H, W = SIZES[case]
    return collections.OrderedDict(c=_head_c("tri." + case, 6, 10, 16), Do=24, H=H, W=W, radius=2)


_HEAD_EXEMPT = {"mask_forms": "no mask operand"}
_HEAD_NOTE = "a head volume's head_stride view is what tests/autograd_contract_table.py covers; here c is strided along its last dim"


def _hold_head(kind, path, module, fn, keys, levels, unit):
    """The yardstick of tests/test_hip_head_stats.py (kind "stats") or tests/test_hip_head_mode.py ("mode") on the clean result."""
    def hold(ops, a, out, dev=None, out_dev=None):
        import importlib
        ref_fn = getattr(importlib.import_module(module), fn)
        operands = tuple(dev[k] for k in keys)
        if kind == "stats":
            from test_hip_head_stats import yardstick
            yardstick(path, "forward contract", out_dev, ref_fn, operands, levels(a))
        else:
            from test_hip_head_mode import Ref, yardstick
            yardstick(path, "forward contract", out_dev, Ref(ref_fn, operands, unit(a)), a["radius"])
    return hold


for _name, _path, _ops, _roles, _rest, _levels, _unit in (
        ("ecm_aggregate9", "eight", _eight, {"c": "head", "w9": "head"}, ("eight_t", "eight_p"), lambda a: a["c"].shape[2], lambda a: a["scale"]),
        ("volume_mapping", "volume", _volume_head, {"c": "head", "m5": "head", "mt3": "head"}, ("volume_t", "volume_p"),
         lambda a: a["c"].shape[2] * a["scale"], lambda a: 1),
        ("trilinear_softargmin", "trilinear", _trilinear, {"c": "head"}, ("trilinear_t3", "trilinear_p"), lambda a: a["Do"], lambda a: 1)):
    _keys = list(_roles) + (["scale"] if _name != "trilinear_softargmin" else ["Do", "H", "W"])
    _row(_name + "_stats", ("odd", "w4"), _ops, _roles,
         (lambda n, keys: lambda ops, a: tuple(getattr(ops, n + "_stats")(*(a[k] for k in keys))))(_name, _keys),
         "test_head_stats_cpu:" + _rest[0], "4 * (the fp32 restatement's error on the device) + 2e-7 max|ref| against fp64, and the ranges: "
         "yardstick of tests/test_hip_head_stats.py", _hold_head("stats", _path, "test_head_stats_cpu", _rest[0], _keys, _levels, _unit),
         batch=(1, 1, 1, 1), exempt=dict(_HEAD_EXEMPT, head_stride=_HEAD_NOTE))
    _row(_name + "_mode", ("odd", "w4"), _ops, _roles,
         (lambda n, keys: lambda ops, a: tuple(getattr(ops, n + "_mode")(*(a[k] for k in keys), a["radius"])))(_name, _keys),
         "test_head_mode_cpu:" + _rest[1], "mode and mass within 4 * e32 + 2e-7 max|ref| about the kernel's own index, the index an argmax "
         "to the stated tolerance: yardstick of tests/test_hip_head_mode.py",
         _hold_head("mode", _path, "test_head_mode_cpu", _rest[1], _keys, _levels, _unit), batch=(1, 1, 1), exempt=dict(_HEAD_EXEMPT, head_stride=_HEAD_NOTE))


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _ulps(a, b):
    key = lambda t: torch.where(_bits32(t) < 0, -(_bits32(t) & 0x7FFFFFFF), _bits32(t)).to(torch.int64)  # noqa: E731
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


# ---- lr_check, the filters, speckle, wls, splat ----------------------------------------------------------------------------------------
def _lr(case):
    from test_disp_warp_cpu import quantised
    H, W = SIZES[case]
    return collections.OrderedDict(disp_l=quantised(B, H, W, 11, top=20), disp_r=quantised(B, H, W, 12, top=20))


def _hold_lr(ops, a, out, dev=None, out_dev=None):
    from test_lr_check_cpu import lr_check_t
    ref = lr_check_t(a["disp_l"].double(), a["disp_r"].double(), 1.0, 0.0, False)
    for name, g, r in zip(("error", "kind", "filled", "src"), out, ref):
        g = g.long() if name == "src" else g.double()
        assert torch.equal(g, r.to(g.dtype)), name


_row("lr_check", ("odd", "w4"), _lr, {"disp_l": "plane", "disp_r": "plane"},
     lambda ops, a: tuple(ops.lr_check(a["disp_l"], a["disp_r"], 1.0, 0.0, with_source=True)),
     "test_lr_check_cpu:lr_check_t", "equal to the fp64 restatement on maps of the 1/64 px grid, where x - d is exact in fp32", _hold_lr,
     batch=(0, 0, 0, 0), exempt={"mask_forms": "no mask operand"})


def _filter(case):
    from test_disp_filter_cpu import float_case
    H, W = SIZES[case]
    d, valid, guide = float_case(1800 + W, (B, H, W), 3)
    return collections.OrderedDict(disp=d, guide=guide, valid=valid)


def _hold_median(ops, a, out, dev=None, out_dev=None):
    from test_disp_filter_cpu import median_t
    for g, w in zip(out, median_t(a["disp"].double(), a["valid"], 2)):
        assert torch.equal(g.double(), w)


_row("disparity_median", ("odd", "w4"), _filter, {"disp": "plane", "valid": "mask"},
     lambda ops, a: tuple(ops.disparity_median(a["disp"], a["valid"], 2, with_support=True)),
     "test_disp_filter_cpu:median_t", "equal to the restatement (the median is one of the inputs)", _hold_median, batch=(0, 0),
     masks={"valid": True})
def _yardstick(K, FLOOR, got, r32, r64, what):
    """|got - fp64| <= K * |fp32 restatement - fp64| + FLOOR * max|fp64|, and equal zero patterns."""
    e32 = float((r32.cpu().double() - r64).abs().max())
    err = float((got.double() - r64).abs().max())
    assert err <= K * e32 + FLOOR * float(r64.abs().max()), (what, err, e32)
    assert torch.equal(got == 0, r64 == 0), what


def _hold_bilateral(ops, a, out, dev=None, out_dev=None):
    from test_disp_filter_cpu import FLOOR, K, bilateral_t
    want = bilateral_t(a["disp"].double(), a["valid"], a["guide"].double(), 2, 1.0, 0.25)
    plain = bilateral_t(dev["disp"], dev["valid"], dev["guide"], 2, 1.0, 0.25)                # the fp32 restatement on the device
    for what, o, o32, o64 in zip(("refined", "weight"), out, plain, want):
        _yardstick(K, FLOOR, o, o32, o64, what)


_row("disparity_bilateral", ("odd", "w4"), _filter, {"disp": "plane", "guide": "guide", "valid": "mask"},
     lambda ops, a: tuple(ops.disparity_bilateral(a["disp"], a["guide"], a["valid"], 2, 1.0, 0.25, with_weight=True)),
     "test_disp_filter_cpu:bilateral_t", "K * (the fp32 restatement's error on the device) + FLOOR max|ref| against fp64, equal zero "
     "patterns, on float_case's inputs (tests/test_hip_disp_filter.py)", _hold_bilateral, batch=(0, 0), masks={"valid": True})


def _speckle(case):
    H, W = SIZES[case]
    d = torch.round(_plane_case("speckle", case, 1.5, 10.0) * 2) / 2
    d[:, 3, 5], d[:, 7, 2] = NAN, float("inf")
    return collections.OrderedDict(disp=d, valid=valid_mask("speckle" + case, (B, H, W)))


def _hold_speckle(ops, a, out, dev=None, out_dev=None):
    from test_disp_speckle_cpu import same_bits, speckle_t
    want = speckle_t(a["disp"], a["valid"], 6, 0.5)
    assert same_bits(out[0], want[0]) and torch.equal(out[1], want[1].to(out[1].dtype)) and torch.equal(out[2], want[2].to(out[2].dtype))


_row("disparity_speckle", ("odd", "w4"), _speckle, {"disp": "plane", "valid": "mask"},
     lambda ops, a: tuple(ops.disparity_speckle(a["disp"], a["valid"], 6, 0.5, with_segments=True)),
     "test_disp_speckle_cpu:speckle_t", "bit-equal", _hold_speckle, batch=(0, 0, 0), masks={"valid": True})


def _wls(case):
    from test_disp_wls_cpu import float_case
    H, W = SIZES[case]
    d, g, conf = float_case(1900 + W, (B, H, W), 3, 0.25, 0.3)
    return collections.OrderedDict(disp=d, guide=g, confidence=conf)


def _hold_wls(ops, a, out, dev=None, out_dev=None):
    from test_disp_wls_cpu import FLOOR, K, wls_t
    ref32 = wls_t(dev["disp"], dev["guide"], dev["confidence"], 200.0, 0.25, 2)
    ref64 = wls_t(a["disp"].double(), a["guide"].double(), a["confidence"].double(), 200.0, 0.25, 2)
    for what, o, r32, r64 in zip(("smoothed", "weight"), out, ref32, ref64):
        assert bool(torch.isfinite(o).all()), what
        _yardstick(K, FLOOR, o, r32, r64, what)


_row("disparity_wls", ("odd", "w4"), _wls, {"disp": "plane", "guide": "guide", "confidence": "plane"},
     lambda ops, a: tuple(ops.disparity_wls(a["disp"], a["guide"], a["confidence"], 200.0, 0.25, 2, with_weight=True)),
     "test_disp_wls_cpu:wls_t", "K * (the fp32 restatement's error on the device) + FLOOR max|ref| against fp64, equal zero patterns, "
     "on float_case's inputs (tests/test_hip_disp_wls.py)", _hold_wls, batch=(0, 0),
     exempt={"mask_forms": "confidence is a weight, not a mask: include/ecm_hip.h multiplies by its value, so a uint8 of 2 or 255 is "
                           "another operand; bool and uint8 are converted by value in ops.py"})


def _splat(case):
    from test_disp_warp_cpu import quantised
    H, W = SIZES[case]
    return collections.OrderedDict(disp=quantised(B, H, W, 21, top=24))


def _hold_splat(ops, a, out, dev=None, out_dev=None):
    from test_disp_splat_cpu import splat_t
    right, src = splat_t(a["disp"])
    assert torch.equal(_bits32(out[0]), _bits32(right)) and torch.equal(out[1].long(), src)


_row("disparity_splat", ("odd", "w4"), _splat, {"disp": "plane"}, lambda ops, a: tuple(ops.disparity_splat(a["disp"], with_source=True)),
     "test_disp_splat_cpu:splat_t", "bit-equal", _hold_splat, batch=(0, 0), exempt={"mask_forms": "no mask operand"})


# ---- reprojection, warp, fuse, motion --------------------------------------------------------------------------------------------------
def _reproject(case):
    H, W = SIZES[case]
    d, Q = scene(case)
    Qs = torch.stack([Q, Q * 1.0, Q]).clone()
    Qs[1, 0, 3] += 0.5                                                     # per-image matrices that differ
    return collections.OrderedDict(disp=d, Q=Qs, attributes=seeded("fc.attrs." + case, B, 2, H, W), valid=valid_mask("reproject" + case, (B, H, W)))


def _hold_cloud(ops, a, out, dev=None, out_dev=None):
    from test_disp_reproject_cpu import cloud_t
    points, offsets, xyz, mask = cloud_t(a["disp"], a["Q"], a.get("attributes"), a["valid"], 0.05, 30.0)[:4]
    if len(out) == 2:
        assert torch.equal(_bits32(out[0]), _bits32(xyz)) and torch.equal(out[1], mask)
    else:
        assert torch.equal(_bits32(out[0]), _bits32(points)) and torch.equal(out[1], offsets)
        assert torch.equal(_bits32(out[2]), _bits32(xyz)) and torch.equal(out[3], mask)


_row("disparity_reproject", ("odd", "w4"), _reproject, {"disp": "plane", "valid": "mask"},
     lambda ops, a: tuple(ops.disparity_reproject(a["disp"], a["Q"], a["valid"], 0.05, 30.0, with_mask=True)),
     "test_disp_reproject_cpu:cloud_t", "bit-equal (cloud_t restates the dense outputs beside the packed ones)", _hold_cloud, batch=(0, 0), matrices=("Q",),
     masks={"valid": True})
_row("point_cloud", ("odd", "w4"), _reproject, {"disp": "plane", "attributes": "guide", "valid": "mask"},
     lambda ops, a: tuple(ops.point_cloud(a["disp"], a["Q"], a["attributes"], a["valid"], 0.05, 30.0, with_dense=True)),
     "test_disp_reproject_cpu:cloud_t", "bit-equal", _hold_cloud, batch=(None, None, 0, 0), matrices=("Q",), masks={"valid": True},
     exempt={"batch:0": "the packed rows are batch-wide: image b's rows are a slice whose place depends on the images before it "
                        "(tests/test_hip_disp_reproject.py holds the concatenation)",
             "batch:1": "offsets are running sums over the batch"})


def _warp(case):
    H, W = SIZES[case]
    d, Q = scene(case)
    import ecm_amd
    M = ecm_amd.ops.warp_matrix(Q, torch.stack([_rigid(0.003, 0.007, -0.002, 0.025, -0.01, 0.03), torch.eye(4, dtype=F64),
                                                _rigid(-0.002, 0.001, 0.003, -0.01, 0.02, 0.0)]))
    return collections.OrderedDict(disp=d, M=M, valid=valid_mask("warp" + case, (B, H, W)), attributes=seeded("fc.wattrs." + case, B, 3, H, W))


def _hold_warp(ops, a, out, dev=None, out_dev=None):
    from test_disp_warp_cpu import warp_t
    want_out, want_src, want_attrs = warp_t(a["disp"], a["M"], a["valid"], a["attributes"], 0.05, 30.0)
    assert torch.equal(_bits32(out[0][:, 0]), _bits32(want_out)) and torch.equal(_bits32(out[1]), _bits32(want_attrs))
    assert torch.equal(out[2][:, 0].long(), want_src)


_row("disparity_warp", ("odd", "w4"), _warp, {"disp": "plane", "valid": "mask", "attributes": "guide"},
     lambda ops, a: tuple(ops.disparity_warp(a["disp"], a["M"], a["valid"], a["attributes"], 0.05, 30.0, with_source=True)),
     "test_disp_warp_cpu:warp_t", "bit-equal", _hold_warp, batch=(0, 0, 0), matrices=("M",), masks={"valid": True})


FUSE_GATE, FUSE_NOISE = 3.0, 0.01


def _fuse(case):
    from test_hip_disp_warp import fusion_inputs                          # planes whose gate decisions cannot depend on fp32 rounding
    H, W = SIZES[case]
    disp, var, prev, pvar, page, source = fusion_inputs((B, H, W), H + W, FUSE_GATE, FUSE_NOISE, True)
    return collections.OrderedDict(disp=disp, var=var, prev=prev, prev_var=pvar, prev_age=page, prev_source=source)


def _hold_fuse(ops, a, out, dev=None, out_dev=None):
    """The rule of test_fusion_decisions_are_exact_and_values_within_four_ulps."""
    from test_disp_warp_cpu import fuse_t
    want_f, want_v, want_age, branch, s, _ = fuse_t(a["disp"], a["var"], a["prev"], a["prev_var"], a["prev_age"], a["prev_source"], FUSE_GATE, FUSE_NOISE, True)
    assert sorted(set(branch.flatten().tolist())) == [0, 1, 3, 4, 5]
    fused, fvar, age = (t[:, 0] for t in out)
    assert torch.equal(age.long(), want_age)
    assert bool((_bits32(fused)[branch == 0] == 0).all()) and bool((_bits32(fvar)[branch == 0] == 0).all())
    copied = (branch == 3) | (branch == 4)
    assert torch.equal(_bits32(fused)[copied], _bits32(a["disp"])[copied]) and torch.equal(_bits32(fvar)[copied], _bits32(a["var"])[copied])
    assert torch.equal(_bits32(fused)[branch == 1], _bits32(a["prev"])[branch == 1])
    live, both = (branch == 1) | (branch == 5), branch == 5
    tol_f = 4 * 2.0 ** -23 * torch.maximum(a["disp"].double().abs(), a["prev"].double().abs())
    tol_v = 4 * 2.0 ** -23 * s
    err_f, err_v = (fused.double() - want_f).abs(), (fvar.double() - want_v).abs()
    assert bool((err_f[both] <= tol_f[both]).all()) and bool((err_v[live] <= tol_v[live]).all())


_row("disparity_fuse", ("odd", "w4"), _fuse, {k: "plane" for k in ("disp", "var", "prev", "prev_var", "prev_age", "prev_source")},
     lambda ops, a: tuple(ops.disparity_fuse(a["disp"], a["var"], a["prev"], a["prev_var"], a["prev_age"], a["prev_source"], FUSE_GATE, FUSE_NOISE, True)),
     "test_disp_warp_cpu:fuse_t", "age and the copied branches exact, fused and variance within four ulps of fp64, on fusion_inputs' planes "
     "(every pixel with a gate margin: tests/test_hip_disp_warp.py)", _hold_fuse, batch=(0, 0, 0), exempt={"mask_forms": "no mask operand"})


def _motion(case):
    H, W = SIZES[case]
    d, Q = scene(case)
    d1 = torch.roll(d, 1, 0) + 0.01
    T = torch.stack([_rigid(0.001, 0.003, 0.0, 0.01, 0.0, 0.02), torch.eye(4, dtype=F64), _rigid(-0.002, 0.001, 0.003, -0.01, 0.02, 0.0)])
    return collections.OrderedDict(disp0=d, disp1=d1, Q=Q, T=T, valid0=valid_mask("m0" + case, (B, H, W)), valid1=valid_mask("m1" + case, (B, H, W), 0.03),
                                   weight=0.5 + torch.rand(B, H, W, generator=torch.Generator().manual_seed(H + W)))


def _hold_motion(ops, a, out, dev=None, out_dev=None):
    from test_motion_align_cpu import align_t
    want = align_t(a["disp0"], a["disp1"], a["Q"], a["T"], valid0=a["valid0"], valid1=a["valid1"], weight=a["weight"])
    sums, res = out[0], out[1][:, 0]
    assert torch.equal(sums[:, 29:], want["sums"][:, 29:])
    assert not bool(((sums - want["sums"]).abs() > want["bound"]).any())
    nan = torch.isnan(want["residual"])
    assert torch.equal(torch.isnan(res), nan) and torch.equal(_bits32(res[~nan]), _bits32(want["residual"][~nan]))


_row("motion_normal", ("odd", "w4"), _motion, {"disp0": "plane", "disp1": "plane", "valid0": "mask", "valid1": "mask", "weight": "plane"},
     lambda ops, a: tuple(ops.motion_normal(a["disp0"], a["disp1"], a["Q"], a["T"], a["valid0"], a["valid1"], a["weight"], with_residual=True)),
     "test_motion_align_cpu:align_t", "the counts equal, every sum within the header's n * 2^-52 * sum |term|, the residual bit-equal",
     _hold_motion, batch=(0, 0), matrices=("T",), masks={"valid0": True, "valid1": True})


# ---- the TSDF volume -------------------------------------------------------------------------------------------------------------------
def _used_volume(dims):
    g = torch.Generator().manual_seed(sum(dims))
    tsdf, wsum, fresh = 2 * torch.rand(dims, generator=g) - 1, 3 * torch.rand(dims, generator=g), torch.rand(dims, generator=g) < 0.33
    return torch.where(fresh, torch.ones(dims), tsdf), torch.where(fresh, torch.zeros(dims), wsum)


def _integrate(case):
    dims = VOLUMES[case]
    origin, voxel = box(dims)
    d, Q = scene("w4")
    tsdf, wsum = _used_volume(dims)
    return collections.OrderedDict(tsdf=tsdf, wsum=wsum, disp=d, Q=Q, T=POSES(), origin=origin, voxel=voxel,
                                   valid=valid_mask("vol" + case, d.shape, 0.05), weight=0.5 + torch.rand(d.shape, generator=torch.Generator().manual_seed(3)))


def _call_integrate(ops, a):
    return tuple(ops.volume_integrate(a["tsdf"], a["wsum"], a["disp"], a["Q"], a["T"], a["origin"], a["voxel"], TRUNC, a["valid"], a["weight"],
                                      max_weight=2.5, min_disp=0.05))


def _hold_integrate(ops, a, out, dev=None, out_dev=None):
    from test_disp_volume_cpu import integrate_t
    m = ops.volume_matrices(a["Q"], a["T"], a["origin"], a["voxel"])
    X, N, touched = integrate_t(a["tsdf"], a["wsum"], a["disp"], a["Q"], m.G, m.C, TRUNC, a["valid"], a["weight"], max_weight=2.5, min_disp=0.05)
    assert max(_ulps(out[0], X), _ulps(out[1], N)) <= 1
    assert torch.equal(_bits32(out[0])[~touched], _bits32(a["tsdf"])[~touched]) and torch.equal(_bits32(out[1])[~touched], _bits32(a["wsum"])[~touched])
    assert 0 < int(touched.sum()) < touched.numel()


_row("volume_integrate", tuple(VOLUMES), _integrate, {"tsdf": "volume", "wsum": "volume", "disp": "plane", "valid": "mask", "weight": "plane"},
     _call_integrate, "test_disp_volume_cpu:integrate_t", "within one ulp of fp32, untouched voxels bit-unchanged", _hold_integrate,
     batch=(0, 0), matrices=("T",), sequential=True, inplace=("tsdf", "wsum"), masks={"valid": True},
     exempt={"strided:volume": "a non-contiguous plane is refused with RuntimeError (the planes are used in place): the refusal and the "
                               "unchanged bits are what the variant checks"})


def _raycast(case):
    from test_disp_volume_cpu import integrate_t
    import ecm_amd
    a = _integrate(case)
    m = ecm_amd.ops.volume_matrices(a["Q"], a["T"], a["origin"], a["voxel"])
    tsdf, wsum, _ = integrate_t(torch.ones(VOLUMES[case]), torch.zeros(VOLUMES[case]), a["disp"], a["Q"], m.G, m.C, TRUNC)
    from test_motion_align_cpu import scene_q
    return collections.OrderedDict(tsdf=tsdf, wsum=wsum, Q_out=scene_q(37, 61), T=a["T"], origin=a["origin"], voxel=a["voxel"], size=(37, 61))


def _call_raycast(ops, a):
    return tuple(ops.volume_raycast(a["tsdf"], a["wsum"], a["Q_out"], a["T"], a["origin"], a["voxel"], a["size"], 10.0, 4.0, 0.5, with_weight=True))


def _hold_raycast(ops, a, out, dev=None, out_dev=None):
    from test_disp_volume_cpu import raycast_t
    m = ops.volume_matrices(a["Q_out"], a["T"], a["origin"], a["voxel"])
    want = raycast_t(a["tsdf"], a["wsum"], m.R, m.Rinv, a["size"], 10.0, 4.0, 0.5)
    o, hw = out[0][:, 0], out[1][:, 0]
    assert torch.equal(o > 0, want["hit"]) and torch.equal(hw > 0, want["hit"]) and bool(want["hit"].any())
    assert max(_ulps(o, want["out"]), _ulps(hw, want["hit_weight"])) <= 1


_row("volume_raycast", tuple(VOLUMES), _raycast, {"tsdf": "volume", "wsum": "volume"}, _call_raycast, "test_disp_volume_cpu:raycast_t",
     "the holes equal as sets, the rest within one ulp of fp32", _hold_raycast, batch=(0, 0), matrices=("T",),
     exempt={"mask_forms": "no mask operand",
             "strided:volume": "a non-contiguous plane is refused with RuntimeError: the refusal is what the variant checks"})


# ---- rectification ---------------------------------------------------------------------------------------------------------------------
def _rectify_map(case):
    from test_rectify_cpu import rig
    import ecm_amd
    K1, D1, K2, D2, R, T, size = rig(5, (48, 64))
    r = ecm_amd.ops.stereo_rectify(K1, D1, K2, D2, R, T, size)
    return collections.OrderedDict(K=K1, D=D1, R=r.R1, P=r.P1, new_size=SIZES[case])


def _hold_rectify_map(ops, a, out, dev=None, out_dev=None):
    from test_rectify_cpu import rectify_map_t
    _, want64 = rectify_map_t(a["K"], a["D"], a["R"], a["P"], a["new_size"])
    got = out[0]
    assert got.shape == (2,) + tuple(a["new_size"]) and bool(torch.isfinite(got).all())
    ulp = torch.exp2(torch.floor(torch.log2(want64.abs().clamp(min=1.0))) - 23)
    assert bool(((got.to(F64) - want64).abs() <= ulp).all())


_NO_TENSOR = "rectify_map takes no tensor operand: its operands are host matrices"
_row("rectify_map", ("odd", "w4"), _rectify_map, {}, lambda ops, a: (ops.rectify_map(a["K"], a["D"], a["R"], a["P"], a["new_size"], "cuda"),),
     "test_rectify_cpu:rectify_map_t", "finite and within one ulp of fp32 of the fp64 map (tests/test_hip_rectify.py)", _hold_rectify_map, batch=(None,),
     exempt={"strided": _NO_TENSOR, "misaligned": _NO_TENSOR, "mask_forms": _NO_TENSOR, "batch": _NO_TENSOR + "; one map per call",
             "batch:0": "one map per call", "untouched": _NO_TENSOR})


def _remap(case):
    from test_rectify_cpu import frames, integer_map
    Ho, Wo = SIZES[case]
    H, W = 23, 36
    g = torch.Generator().manual_seed(Wo)
    mp = lambda: torch.stack([integer_map(Ho, Wo)[0] * (W - 1) / (Wo - 1), integer_map(Ho, Wo)[1] * (H - 1) / (Ho - 1)]).expand(B, 2, Ho, Wo) \
        + 0.8 * torch.rand(B, 2, Ho, Wo, generator=g) - 0.9                # noqa: E731  (sub-pixel coordinates, some outside the source)
    return collections.OrderedDict(left_raw=frames(B, H, W, 5), right_raw=frames(B, H, W, 6), map_left=mp().contiguous(), map_right=mp().contiguous())


def _hold_remap(ops, a, out, dev=None, out_dev=None):
    from test_rectify_cpu import remap_t
    for raw, mp, got, mask in ((a["left_raw"], a["map_left"], out[0], out[3]), (a["right_raw"], a["map_right"], out[1], out[4])):
        want64, _, want_mask = remap_t(raw, mp, border=23.0)
        want32 = remap_t(raw, mp, border=23.0, dtype=F32)[0]
        assert torch.equal(mask, want_mask)
        assert float((got.to(F64) - want64).abs().max()) <= 4 * float((want32.to(F64) - want64).abs().max())


_row("remap_pair", ("odd", "w4"), _remap, {"left_raw": "image", "right_raw": "image", "map_left": "plane", "map_right": "plane"},
     lambda ops, a: tuple(ops.remap_pair(a["left_raw"], a["right_raw"], a["map_left"], a["map_right"], border=23.0, want_image=True, with_mask=True)),
     "test_rectify_cpu:remap_t", "masks equal, the planes within four times the fp32 restatement's own error from fp64", _hold_remap,
     batch=(0, 0, 0, 0, 0), exempt={"mask_forms": "no mask operand (the masks are outputs)",
                                    "four_dim": "the maps are [2,Ho,Wo] or [B,2,Ho,Wo]: there is no second form of one shape"})


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
def _eval(case):
    from test_sparsification_cpu import random_case
    H, W = SIZES[case]
    pred, gt = random_case(60 + W, (B, H, W))
    return collections.OrderedDict(pred=pred, gt=gt)


def _sparsify(case):
    a = _eval(case)
    noise = seeded("fc.sp.noise." + case, *a["pred"].shape)
    a["m0"], a["m1"] = noise * 3, (a["pred"] - a["gt"]).abs() + noise.abs()
    return a


def _table_of(sp):
    return torch.cat([torch.stack([sp.epe, sp.d1], -1), torch.stack([sp.oracle_epe, sp.oracle_d1], -1).unsqueeze(1)], 1)


def _call_sparsify(ops, a):
    sp = ops.eval_sparsification(a["pred"], a["gt"], [a["m0"], a["m1"]], 192, 7)
    return (_table_of(sp), sp.count, sp.ause_epe, sp.ause_d1, sp.aurg_epe, sp.aurg_d1)


def _hold_sparsify(ops, a, out, dev=None, out_dev=None):
    from test_sparsification_cpu import sparsify_t
    table, count = sparsify_t(a["pred"], a["gt"], [a["m0"], a["m1"]], 192, 7)
    nan = torch.isnan(table)
    assert torch.equal(out[1], count) and torch.equal(torch.isnan(out[0]), nan)
    assert int((_bits32(out[0]).long() - _bits32(table).long())[~nan].abs().max()) <= 1


_row("eval_sparsification", ("odd", "w4"), _sparsify, {"pred": "plane", "gt": "plane", "m0": "plane", "m1": "plane"}, _call_sparsify,
     "test_sparsification_cpu:sparsify_t", "the counts equal, the table within one ulp of fp32", _hold_sparsify, batch=(0,) * 6,
     exempt={"mask_forms": "no mask operand", "four_dim:gt": "gt is [B,H,W] only; pred and the measures take both forms"})
_BATCH_WIDE = "the row is a mean over the whole batch, not a stack of per-image rows"
def _eval_kitti(case):
    from test_hip_eval_kitti import random_case
    H, W = SIZES[case]
    pred, gt = random_case(B, H, W, 70 + W)
    return collections.OrderedDict(pred=pred, gt=gt)


def _hold_kitti(ops, a, out, dev=None, out_dev=None):
    from test_hip_eval_kitti import check_row
    fails = []
    check_row("kitti.contract", "row", out[0], a["pred"], a["gt"], fails)
    for b in range(B):
        check_row("kitti.contract", f"table[{b}]", out[1][b], a["pred"][b:b + 1], a["gt"][b:b + 1], fails)
    assert out[1][:, 4:].double().sum(0).tolist() == out[0][4:].double().tolist()
    assert not fails, "\n".join(fails)


def _hold_epe(ops, a, out, dev=None, out_dev=None):
    """The rule of tests/test_hip_metrics_fp64.py::test_eval_epe_fp64."""
    from test_costvol_geometry import epe_reference
    from test_hip_metrics_fp64 import yardstick
    H, W = a["pred"].shape[-2:]
    means, counts, err, masks = epe_reference(a["pred"], a["gt"], H - 1, W - 2)
    got, fails = out[0], []
    assert [float(v) for v in got[3:]] == [float(v) for v in counts]
    err_dev = err.to("cuda")
    for k, what in enumerate(("epe", "epe_non", "epe_true")):
        if counts[k] == 0:
            assert bool(torch.isnan(got[k])), what
            continue
        yardstick("epe.contract", "row", what, got[k], means[k], [torch.mean(err[masks[k]]), torch.mean(err_dev[masks[k].to("cuda")])], fails)
    assert not fails, "\n".join(fails)


_row("eval_kitti", ("odd", "w4"), _eval_kitti, {"pred": "plane", "gt": "plane"}, lambda ops, a: tuple(ops.eval_kitti(a["pred"], a["gt"], per_sample=True)),
     "test_eval_kitti_cpu:restate64", "counts and loss_3 equal, the means within the fp64 yardstick: check_row of tests/test_hip_eval_kitti.py, "
     "for the row and every row of the table", _hold_kitti, batch=(None, 0), exempt={"mask_forms": "no mask operand", "batch:0": _BATCH_WIDE + "; the per-sample table is held",
                                                "four_dim:gt": "gt is [B,H,W] only; pred takes both forms"})
_row("eval_epe", ("odd", "w4"), _eval, {"pred": "plane", "gt": "plane"},
     lambda ops, a: (ops.eval_epe(a["pred"], a["gt"], a["pred"].shape[-2] - 1, a["pred"].shape[-1] - 2),),
     "test_costvol_geometry:epe_reference", "counts equal, the means within the fp64 yardstick (tests/test_hip_metrics_fp64.py)", _hold_epe,
     batch=(None,),
     exempt={"mask_forms": "no mask operand", "batch": _BATCH_WIDE, "batch:0": _BATCH_WIDE,
             "four_dim:gt": "gt is [B,H,W] only; pred takes both forms"})


def _hold_u16(ops, a, out, dev=None, out_dev=None):
    import warnings
    import numpy as np
    import oracle.ecm_oracle as O
    H, W = a["pred"].shape[-2:]
    img = out[0].numpy()
    for b in range(B):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = O.kitti_disparity_uint16(a["pred"][b:b + 1], H - 1, W - 2)
        assert np.array_equal(img[b], want), b


_row("disparity_to_uint16", ("odd", "w4"), lambda case: collections.OrderedDict(pred=_plane_case("u16", case, 20.0, 0.0).abs() + 1.0), {"pred": "plane"},
     lambda ops, a: (ops.disparity_to_uint16(a["pred"], [a["pred"].shape[-2] - 1] * a["pred"].shape[0], [a["pred"].shape[-1] - 2] * a["pred"].shape[0]),),
     "oracle.ecm_oracle:kitti_disparity_uint16", "equal to the numpy cast, sample by sample", _hold_u16, batch=(0,),
     exempt={"mask_forms": "no mask operand"})


def four_dim_operands(name):
    """The operands of a row that take both [B,H,W] and [B,1,H,W]: its planes and masks that are built as [B,H,W]."""
    row = ROWS[name]
    if "four_dim" in row.exempt:
        return ()
    return tuple(k for k, r in row.roles.items() if r in ("plane", "mask") and f"four_dim:{k}" not in row.exempt)
