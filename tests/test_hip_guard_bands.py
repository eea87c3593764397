"""Guard bands: every buffer the ops layer hands to the C ABI as an OUTPUT or as SCRATCH -- forward and
backward, every entry point -- is carved out of a larger allocation whose margins (1 MiB on either side) are poisoned; after
the kernels have run the margins must be intact.  An out-of-bounds store at a ragged shape (the class of bug that an
intermittent abort such as round 2's `r2_t8.log` points at) then fails deterministically in the test that causes it, instead
of corrupting a neighbour's memory and surfacing later or never.

Mechanism: `ops` allocates with `torch.empty` / `torch.empty_like` / `torch.zeros`; for the duration of a case the module's
`torch` name is replaced by a proxy whose allocation functions return guarded views (everything else is forwarded)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
MARGIN = 1 << 20
POISON = 0xA5


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


class _GuardedTorch:
    def __init__(self):
        self.records = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device):
        dtype = dtype or torch.float32
        if device is None or torch.device(device).type != "cuda":
            return torch.empty(shape, dtype=dtype, device=device)
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((nbytes + 2 * MARGIN + 512,), POISON, dtype=torch.uint8, device=device)
        off = MARGIN + (-(raw.data_ptr() + MARGIN)) % 256
        self.records.append((raw, off, nbytes))
        return raw[off:off + nbytes].view(dtype).view(tuple(int(d) for d in shape))

    def empty(self, *size, dtype=None, device=None, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return self._alloc(tuple(shape), dtype, device)

    def empty_like(self, t, **kw):
        return self._alloc(tuple(t.shape), t.dtype, t.device)

    def zeros(self, *size, dtype=None, device=None, **kw):
        out = self.empty(*size, dtype=dtype, device=device)
        out.zero_()
        return out

    def check(self, what):
        torch.cuda.synchronize()
        assert self.records, f"{what}: no guarded allocation was made (the proxy is not in the allocation path)"
        for i, (raw, off, n) in enumerate(self.records):
            lo, hi = raw[:off], raw[off + n:]
            assert bool((lo == POISON).all()), f"{what}: allocation {i} ({n} bytes): store BELOW the buffer"
            assert bool((hi == POISON).all()), f"{what}: allocation {i} ({n} bytes): store PAST the end of the buffer"


@contextlib.contextmanager
def guarded(ecm):
    ops = ecm.ops
    proxy = _GuardedTorch()
    real = ops.torch
    ops.torch = proxy
    try:
        yield proxy
    finally:
        ops.torch = real


def R(*shape, seed=0, scale=1.0, grad=True):
    t = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) * scale
    return t.requires_grad_() if grad else t


def _bw(y):
    ys = y if isinstance(y, (tuple, list)) else (y,)
    sum((t * torch.randn_like(t)).sum() for t in ys if t.requires_grad).backward()


_CONV3 = [(1, 6, 10, (3, 5, 7)), (2, 32, 32, (5, 7, 70)), (1, 64, 64, (3, 9, 33)), (1, 32, 64, (2, 4, 130)), (1, 8, 12, (3, 5, 9)),
          (1, 32, 32, (1, 1, 2)), (1, 64, 32, (6, 13, 65)), (1, 4, 4, (2, 3, 2)), (1, 16, 16, (1, 3, 127)), (1, 8, 8, (1, 4, 129)),
          (1, 32, 32, (7, 9, 31)), (2, 32, 1, (4, 6, 37)), (1, 24, 1, (5, 5, 66))]


@pytest.mark.parametrize("B,Ci,Co,dims", _CONV3)
@pytest.mark.parametrize("wino", [True, False])
def test_conv3d_all_paths(ecm, B, Ci, Co, dims, wino):
    """Conv3d k3 stride 1: forward, data gradient (+ skip addend through the fork), weight gradient -- Winograd and direct."""
    ops = ecm.ops
    if not wino and (Ci % 4 or Co > 64):
        pytest.skip("outside the direct kernel's contract")
    prev = ops.WINOGRAD
    ops.WINOGRAD = wino
    try:
        with guarded(ecm) as g:
            x, w = R(B, Ci, *dims, seed=1), R(Co, Ci, 3, 3, 3, seed=2, scale=0.1)
            y, xs = ops.conv3d_k3(x, w, 1, fork=True)
            _bw((y, xs))
            g.check(f"conv3d {B}x{Ci}->{Co} {dims} wino={wino}")
    finally:
        ops.WINOGRAD = prev


@pytest.mark.parametrize("B,Ci,Co,dims", [(1, 32, 64, (5, 7, 9)), (2, 32, 64, (8, 12, 66)), (1, 64, 64, (6, 10, 34)), (1, 64, 64, (3, 3, 3)),
                                          (1, 32, 64, (12, 36, 60))])
def test_stride2_conv_and_transposed_conv(ecm, B, Ci, Co, dims):
    ops = ecm.ops
    with guarded(ecm) as g:
        x, w = R(B, Ci, *dims, seed=3), R(Co, Ci, 3, 3, 3, seed=4, scale=0.1)
        _bw(ops.conv3d_k3(x, w, 2))
        g.check(f"conv3d stride 2 {dims}")
    with guarded(ecm) as g:
        x, w = R(B, Co, *dims, seed=5), R(Co, Ci, 3, 3, 3, seed=6, scale=0.1)
        _bw(ops.deconv3d_k3s2(x, w))
        g.check(f"deconv3d {dims}")


@pytest.mark.parametrize("shape,skip,relu", [((2, 32, 5, 7, 9), False, True), ((1, 64, 3, 6, 10), True, True), ((3, 32, 1, 1, 2), False, False),
                                             ((1, 32, 48, 36, 60), True, False), ((2, 128, 9, 15), False, True), ((4, 32, 48, 144, 240), False, True)])
@pytest.mark.parametrize("cluster", [1, 0])
def test_groupnorm(ecm, shape, skip, relu, cluster):
    ops = ecm.ops
    prev = ops.gn_cluster_mode(cluster)
    try:
        with guarded(ecm) as g:
            x = R(*shape, seed=7)
            gm, bt = R(shape[1], seed=8), R(shape[1], seed=9)
            sk = R(*shape, seed=10) if skip else None
            _bw(ops.group_norm_act(x, gm, bt, sk, relu))
            g.check(f"groupnorm {shape} skip={skip} relu={relu} cluster={cluster}")
    finally:
        ops.gn_cluster_mode(prev)
    ops.check_async_errors()


_C2 = [(2, 3, 32, 20, 41, 3, 1, 1), (1, 32, 32, 33, 70, 3, 1, 1), (2, 32, 32, 34, 66, 3, 2, 1), (1, 32, 32, 21, 37, 3, 2, 1), (1, 64, 128, 16, 40, 3, 1, 1),
       (1, 128, 128, 20, 36, 3, 1, 2), (1, 128, 128, 24, 40, 3, 1, 4), (1, 320, 128, 12, 36, 3, 1, 1), (2, 32, 64, 16, 34, 1, 2, 1), (1, 64, 128, 15, 33, 1, 1, 1),
       (8, 128, 32, 2, 3, 1, 1, 1), (1, 64, 64, 9, 3, 3, 1, 1)]


@pytest.mark.parametrize("B,Ci,Co,H,W,k,stride,dil", _C2)
def test_conv2d_family(ecm, B, Ci, Co, H, W, k, stride, dil):
    ops = ecm.ops
    with guarded(ecm) as g:
        x, w = R(B, Ci, H, W, seed=11), R(Co, Ci, k, k, seed=12, scale=0.1)
        if stride == 1 and k == 3 and dil == 1:
            y, xs = ops.conv2d(x, w, stride, dil, fork=True)
            _bw((y, xs))
        else:
            _bw(ops.conv2d(x, w, stride, dil))
        g.check(f"conv2d {Ci}->{Co} {H}x{W} k{k} s{stride} d{dil}")


def test_dilated_phase_planes_and_class_convolutions(ecm):
    ops = ecm.ops
    with guarded(ecm) as g:
        x, w = R(1, 128, 4, 9, 17, seed=13), R(128, 128, 3, 3, seed=14, scale=0.05)
        y, xs = ops.conv2d_planes(x, w, fork=True)
        _bw((y, xs))
        g.check("conv2d_planes")
    with guarded(ecm) as g:
        L, Rr, w = R(2, 32, 9, 33, seed=15), R(2, 32, 9, 33, seed=16), R(32, 64, 3, 3, 3, seed=17, scale=0.1)
        _bw(ops.costvol_conv3d(L, Rr, w, 12))
        g.check("costvol_conv3d")
    with guarded(ecm) as g:
        L, Rr = R(2, 8, 5, 24, seed=18), R(2, 8, 5, 24, seed=19)
        _bw(ops.cost_volume(L, Rr, 20))
        g.check("cost_volume")


@pytest.mark.parametrize("B,h,w", [(1, 3, 5), (2, 7, 13), (2, 144, 240)])
def test_ecm_weights_heads_and_loss(ecm, B, h, w):
    """ecm_weights9 forward + backward (B=2 at 576x960 is the case `r2_t8.log` aborted in), soft-argmin, aggregation, loss."""
    ops = ecm.ops
    Ws = [R(*s, seed=20 + i, scale=0.2) for i, s in enumerate(((32, 66, 1, 1), (16, 32, 1, 1), (8, 16, 1, 1), (1, 8, 1, 1)))]
    with guarded(ecm) as g:
        lr, hr = R(B, 32, h, w, seed=24), R(B, 32, 4 * h, 4 * w, seed=25)
        w9 = ops.ecm_weights9(lr, hr, *Ws)
        c = R(3, B, 12, h, w, seed=26)
        preds = ops.ecm_aggregate9(ops.softargmin_heads(c), w9, 4)
        gt = torch.rand(B, 4 * h, 4 * w, device="cuda") * 191.0
        loss, _ = ops.stereo_loss3([preds[0], preds[1], preds[2]], gt)
        loss.backward()
        ops.eval_epe(preds[2].detach(), gt, min(540, 4 * h), min(960, 4 * w))
        ops.disparity_to_uint16(preds[2].detach(), 4 * h - 1, 4 * w - 2)
        g.check(f"ecm weights / heads / loss B={B} {h}x{w}")


@pytest.mark.parametrize("s,h,w", [(8, 3, 5), (16, 2, 3), (8, 9, 17)])
def test_variant_heads(ecm, s, h, w):
    ops = ecm.ops
    Ws = [R(*sh, seed=30 + i, scale=0.2) for i, sh in enumerate(((32, 66, 1, 1), (16, 32, 1, 1), (8, 16, 1, 1), (1, 8, 1, 1)))]
    with guarded(ecm) as g:
        lr, hr = R(2, 32, h, w, seed=34), R(2, 32, s * h, s * w, seed=35)
        m5, mt3 = ops.context_weights(lr, hr, *Ws, 1), ops.context_weights(lr, hr, *Ws, 2)
        c = R(3, 2, 192 // s, h, w, seed=36)
        _bw(ops.volume_mapping(c, m5, mt3, s))
        g.check(f"context weights + volume mapping s={s}")
    with guarded(ecm) as g:
        c = R(3, 2, 192 // s, h, w, seed=37)
        _bw(ops.trilinear_softargmin(c, 192, s * h + 3, s * w - 1))
        g.check(f"trilinear head s={s}")


def test_frame_preparation(ecm):
    ops = ecm.ops
    with guarded(ecm) as g:
        frames = torch.rand(2, 300, 530, 7, device="cuda") * 255.0
        ops.frame_prep(frames, [3, 44], [0, 18], 256, 512, want_image=True)
        ops.frame_prep(torch.rand(1, 540, 960, 7, device="cuda"), [0], [0], 576, 960, split=540, tail=36)
        ops.frame_prep_kitti_eval(torch.rand(1, 375, 1242, 7, device="cuda"))
        rgb = (torch.rand(2, 300, 530, 6, device="cuda") * 255).to(torch.uint8)
        ops.frame_prep((rgb, torch.rand(2, 300, 530, device="cuda").half()), [1, 2], [3, 4], 256, 512)
        g.check("frame_prep")


# ---- the weight gradients' scratch: what the query promises against what the launcher writes -----------------------------------------
# kind -> (query, entry point, family of the restated plan); a case is (kind, B, Ci, Co, (D, H, W) of x, kh = kw, stride)
_WG = {"3d": ("ecm_conv3d_wgrad_scratch_bytes", "ecm_conv3d_k3_wgrad"), "wino": ("ecm_conv_wino_wgrad_scratch_bytes", "ecm_conv_wino_wgrad"),
       "2d": ("ecm_conv2d_wgrad_ex_scratch_bytes", "ecm_conv2d_wgrad_ex"), "c1": ("ecm_conv3d_c1_wgrad_scratch_bytes", "ecm_conv3d_c1_wgrad"),
       "c1gn": ("ecm_conv3d_c1_wgrad_scratch_bytes", "ecm_conv3d_c1_gn_wgrad"), "c1_2d": ("ecm_conv2d_c1_wgrad_scratch_bytes", "ecm_conv2d_c1_wgrad")}
_WG_CAP = [("3d", 1, 64, 64, (6, 32, 96), 3, 1), ("3d", 1, 64, 64, (12, 32, 96), 3, 2), ("wino", 1, 64, 64, (6, 32, 96), 3, 1),
           ("wino", 1, 128, 128, (1, 90, 90), 1, 1), ("2d", 1, 128, 128, (1, 90, 90), 3, 1), ("2d", 1, 128, 128, (1, 140, 140), 1, 2)]
_WG_REFUSE = _WG_CAP[:1] + _WG_CAP[3:5] + [("c1", 2, 32, 1, (6, 9, 33), 3, 1), ("c1gn", 2, 32, 1, (6, 9, 33), 3, 1), ("c1_2d", 2, 8, 1, (1, 40, 70), 3, 1)]


def _wg_setup(ecm, case, alloc):
    """-> (sizes of the query, entry point, its arguments with ops._SCRATCH in place, gw, (ntiles, P) of the restated plan).  The
    operands come from torch, the outputs from `alloc` (the guarded proxy's `empty` inside `guarded`)."""
    import test_wgrad_plan_cpu as WP
    ops = ecm.ops
    kind, B, Ci, Co, (D, H, W), k, stride = case
    p, st = ops._p, ops._stream()
    Do, Ho, Wo = ((n - 1) // stride + 1 for n in (D, H, W))
    x = R(B, Ci, D, H, W, seed=40, grad=False)
    gy = R(B, Co, Do, Ho, Wo, seed=41, grad=False)
    query, entry = _WG[kind]
    if kind == "3d":
        gw = alloc(Co, Ci, 3, 3, 3, device="cuda")
        return (B, Ci, Co, D, H, W, stride), entry, (p(x), p(gy), p(gw), ops._SCRATCH, B, Ci, Co, D, H, W, stride, st), gw, \
            (x, gy), WP.plan_3d(B, Ci, Co, D, H, W, stride)[:2]
    if kind == "wino":
        gw = alloc(Co, Ci, k, 3, 3, device="cuda")
        return (B, Ci, Co, D, H, W, k), entry, (p(x), p(gy), p(gw), ops._SCRATCH, B, Ci, Co, D, H, W, k, st), gw, \
            (x, gy), WP.plan_wino(B, Ci, Co, D, H, W, k)[:2]
    if kind == "2d":
        gw = alloc(Co, Ci, k, k, device="cuda")
        return (B, Ci, Co, Ho, Wo, k, k, stride), entry, \
            (p(x), p(gy), p(gw), ops._SCRATCH, B, Ci, Co, H, W, k, k, stride, 1, k // 2, k // 2, Ho, Wo, st), gw, \
            (x, gy), WP.plan_2d(B, Ci, Co, Ho, Wo, k, k, stride)[:2]
    if kind in ("c1", "c1gn"):
        gw = alloc(1, Ci, 3, 3, 3, device="cuda")
        gn = (torch.rand(B, 32, 2, device="cuda") + 0.5, R(Ci, seed=42, grad=False), R(Ci, seed=43, grad=False)) if kind == "c1gn" else ()
        return (B, Ci, D, H, W), entry, (p(x), *map(p, gn), p(gy), p(gw), ops._SCRATCH, B, Ci, D, H, W, st), gw, \
            (x, gy, gn), WP.plan_c1_3d(B, Ci, D, H, W)[:2]
    gw, gb = alloc(1, Ci, 3, 3, device="cuda"), alloc(1, device="cuda")      # c1_2d: x, gy, y (the layer's ReLU output), gw, gb
    y = R(B, 1, H, W, seed=44, grad=False)
    return (B, Ci, H, W), entry, (p(x), p(gy), p(y), p(gw), p(gb), ops._SCRATCH, B, Ci, H, W, st), gw, (x, gy, y, gb), \
        WP.plan_c1_2d(B, Ci, H, W)[:2]


@pytest.mark.parametrize("case", _WG_CAP, ids=lambda c: "%s-k%d-s%d-%dx%d" % (c[0], c[5], c[6], c[2], c[3]))
def test_weight_gradient_where_the_worker_cap_binds(ecm, case):
    """P < ntiles: every worker walks several tiles and the scratch is P partials, not one per tile.  The scratch these calls get
    is exactly the queried size (ops._call_scratch allocates it through the guarded proxy), so intact margins show that the query
    and the launcher read one plan."""
    ops = ecm.ops
    with guarded(ecm) as g:
        sizes, entry, args, gw, keep, (ntiles, P) = _wg_setup(ecm, case, ops.torch.empty)
        assert P < ntiles, f"{case}: the worker cap no longer binds ({P} workers, {ntiles} tiles)"
        ops._call_scratch("cuda", _WG[case[0]][0], sizes, entry, *args)
        g.check(f"weight gradient {case}")
        assert len(g.records) == 2 and bool(torch.isfinite(gw).all())       # gw and the scratch
    ops.check_async_errors()


@pytest.mark.parametrize("case", _WG_REFUSE, ids=lambda c: "%s-k%d-s%d" % (c[0], c[5], c[6]))
def test_weight_gradient_refuses_short_scratch(ecm, case):
    """One byte short of the query: ECM_ESCRATCH (-3) through the C ABI, nothing launched, the output untouched."""
    import ctypes
    ops = ecm.ops
    sizes, entry, args, gw, keep, _ = _wg_setup(ecm, case, torch.empty)
    nb = ecm._lib.query(_WG[case[0]][0], *sizes)
    assert nb > 16
    gw.fill_(777.0)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    at = next(i for i, a in enumerate(args) if a is ops._SCRATCH)
    fn = getattr(ecm._lib.load(), entry)
    assert fn(*args[:at], ops._p(scratch), ctypes.c_longlong(nb - 1), *args[at + 1:]) == -3
    torch.cuda.synchronize()
    assert bool((gw == 777.0).all())
    ops.check_async_errors()


def test_the_proxy_catches_an_out_of_bounds_store(ecm):
    """The fixture itself: a store one element past a guarded buffer is reported."""
    with guarded(ecm) as g:
        t = ecm.ops.torch.empty(4, 8, device="cuda", dtype=torch.float32)
        raw, off, n = g.records[0]
        raw[off + n:off + n + 4] = 0                       # what a kernel writing element [4*8] would do
        with pytest.raises(AssertionError, match="PAST the end"):
            g.check("self-test")
        assert t.shape == (4, 8)
