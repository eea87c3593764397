"""What ops.py actually hands to the C ABI: every call that goes through ecm_amd._lib.call / _lib.query while the models and
the standalone ops run is recorded and each argument is checked, by position, against PROTOTYPES[name][1].  ctypes converts a
Python value to the declared C type without a range check (an int beyond 32 bits wraps silently in a c_int parameter), so the
values are checked here, before ctypes sees them.  tests/test_abi_types.py holds the table to the header; the fp64 suites own the
numerics: nothing here asserts a result.  The wrapper forwards every call unchanged.

The closing test reads the union of the entry points the module recorded: recorded + ABI_ONLY (tests/test_abi_types.py) must be
exactly PROTOTYPES, so every row is either exercised with checked arguments or accounted for by name."""
import contextlib
import ctypes as C
import math

import pytest
import torch

from test_abi_types import ABI_ONLY

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = W = 256            # the smallest frame every pyramid depth accepts (tests/test_hip_disp_filter.py::test_refine_256x256)
ARCHS = ("cmfsm", "cmfsm_sub_8", "cmfsm_sub_16", "cm_sub_4", "cm_sub_8", "cm_sub_16", "bilinear_cmf", "bilinear_cmf_sub_8",
         "bilinear_cmf_sub_16", "cmf")
SPLIT_ALL = ("conv_fwd", "conv_dgrad", "deconv_fwd", "deconv_dgrad")

# Alignment that the header demands of a device pointer (include/ecm_hip.h: "16-byte aligned pointers"); every other tensor
# operand must be aligned to its element, and what went through ops._c to 16 bytes (the promise in its docstring).
ALIGN = {"ecm_sum_n": 16}

RECORDED = set()       # entry points seen by any case of this module, for the closing test
INT_MAX = {}           # name -> (largest _I argument, its index): printed by the closing test (ABI section)
CASES = set()          # the driver cases that ran


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    assert sorted(ecm_amd.models._MODELS) == sorted(ARCHS)        # "every registered architecture"
    return ecm_amd


def check_arguments(name, args, argtypes, tensors, problems, census=True):
    """Append to `problems` what is wrong with `args` as the arguments of entry point `name`.  census: feed INT_MAX."""
    if len(args) != len(argtypes):
        problems.append(f"{name}: {len(args)} arguments for {len(argtypes)} parameters")
        return
    for i, (v, t) in enumerate(zip(args, argtypes)):
        at = f"{name} argument {i}"
        if t is C.c_int:
            if type(v) is not int:
                problems.append(f"{at}: c_int takes a plain int, got {type(v).__name__} {v!r}")
            elif not -2 ** 31 <= v < 2 ** 31:
                problems.append(f"{at}: {v} does not fit a c_int")
            elif census and v > INT_MAX.get(name, (-1, 0))[0]:
                INT_MAX[name] = (v, i)
        elif t is C.c_longlong:
            w = v.value if type(v) is C.c_longlong else v
            if type(w) is not int or not -2 ** 63 <= w < 2 ** 63:
                problems.append(f"{at}: c_longlong takes an int or a c_longlong, got {type(v).__name__} {v!r}")
        elif t is C.c_float:
            if type(v) not in (float, int) or not math.isfinite(v):
                problems.append(f"{at}: c_float takes a finite float or int, got {type(v).__name__} {v!r}")
        elif t is C.c_void_p:
            if not (v is None or type(v) is int or type(v) is C.c_void_p):
                problems.append(f"{at}: a pointer is None, an int or a c_void_p, got {type(v).__name__}")
                continue
            meta = tensors.get(id(v))
            if meta is None or not meta[1]:
                continue                                          # NULL, a stream, a host array: nothing more to know
            _, ptr, elem, contiguous, cuda, promised16 = meta
            need = max(elem, ALIGN.get(name, 1), 16 if promised16 else 1)
            if not cuda:
                problems.append(f"{at}: a host tensor's address")
            if not contiguous:
                problems.append(f"{at}: the address of a tensor that is not contiguous")
            if ptr % need:
                problems.append(f"{at}: address {ptr:#x} is not aligned to {need} bytes")
        else:
            problems.append(f"{at}: parameter type {t} has no rule here")


@contextlib.contextmanager
def recording(ecm, case, table=None, census=True, strict=False):
    """Wrap _lib.call and _lib.query (and ops._p / ops._c, to know which addresses are tensors and which were promised
    aligned) for the block; on exit every recorded call has been checked and the device has reported no asynchronous error.
    table: the table of _lib.TABLES whose calls are recorded and checked (default PROTOTYPES); a name of another table passes
    through, a name of none is a problem.  Only PROTOTYPES feeds this module's closing test (RECORDED, CASES, INT_MAX).
    census=False: the block is another module's (tests/test_hip_autograd_contract.py): RECORDED, CASES and INT_MAX are left alone,
    strict=True: a call whose arguments have a problem
    raises AssertionError, with the argument named, BEFORE it is forwarded -- nothing is launched on a bad pointer."""
    lib, ops = ecm._lib, ecm.ops
    table = lib.PROTOTYPES if table is None else table
    own = census and table is lib.PROTOTYPES
    real_call, real_query, real_p, real_c = lib.call, lib.query, ops._p, ops._c
    calls, problems, tensors, aligned = [], [], {}, set()

    def record(name, args):
        if name in table:
            calls.append(name)
            seen = len(problems)
            check_arguments(name, args, table[name][1], tensors, problems, census)
            if census and not own:
                INT_MAX.pop(name, None)                            # the table of largest ints is about this module's cases
            if strict and len(problems) > seen:
                raise AssertionError(f"{case}: refused before the call:\n" + "\n".join(problems[seen:]))
        elif not any(name in t for t, _ in lib.TABLES.values()):
            problems.append(f"{name}: in no table")
            if strict:
                raise AssertionError(f"{case}: {problems[-1]}")

    def call(name, *args):
        record(name, args)
        return real_call(name, *args)

    def query(name, *args):
        record(name, args)
        return real_query(name, *args)

    def _c(t):
        out = real_c(t)
        aligned.add(out.data_ptr())
        return out

    def _p(t):
        p = real_p(t)
        if t is not None:                                          # the c_void_p object is kept, so its id stays its own
            tensors[id(p)] = (p, t.data_ptr(), t.element_size(), t.is_contiguous(), t.is_cuda, t.data_ptr() in aligned)
        return p

    lib.call, lib.query, ops._p, ops._c = call, query, _p, _c
    try:
        yield calls
        ops.check_async_errors()                                   # inside the wrapper: ecm_async_status is an entry point too
    finally:
        lib.call, lib.query, ops._p, ops._c = real_call, real_query, real_p, real_c
    assert calls, "nothing went through _lib.call"
    assert not problems, f"{len(problems)} bad arguments, the first 20:\n" + "\n".join(problems[:20])
    if own:
        RECORDED.update(calls)
        CASES.add(case)


_models = {}


def _model(ecm, arch):
    if arch not in _models:
        torch.manual_seed(5)
        _models[arch] = ecm.get_model(arch).to(DEV)
    return _models[arch]


def _pair(seed=11):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(1, 3, H, W, device=DEV, generator=gen), torch.randn(1, 3, H, W, device=DEV, generator=gen)


def _gt(seed=8):
    return (torch.rand(1, H, W, generator=torch.Generator().manual_seed(seed)) * 191.0).to(DEV)


def _train_step(ecm, model, left, right, gt):
    with torch.enable_grad():
        model.zero_grad(set_to_none=True)
        loss, _ = ecm.ops.stereo_loss3(model(left, right), gt, 192)
        loss.backward()
        ecm.ops.join_side_streams()


@pytest.mark.parametrize("arch", ARCHS)
def test_training_step(ecm, arch):
    model, (left, right) = _model(ecm, arch).train(), _pair()
    with recording(ecm, f"train:{arch}") as calls:
        _train_step(ecm, model, left, right, _gt())
    assert "ecm_stereo_loss_fwd" in calls and "ecm_stereo_loss_bwd" in calls


@pytest.mark.parametrize("arch", ARCHS)
def test_inference_methods(ecm, arch):
    model, (left, right) = _model(ecm, arch).eval(), _pair()
    with_distribution = model.HEAD not in ecm.models._NO_DISTRIBUTION      # predict / sparsification exist for these heads
    with recording(ecm, f"infer:{arch}") as calls:
        if with_distribution:
            model.predict(left, right, mode_radius=model.LEVEL_SPACING)
            model.sparsification(left, right, _gt(), mode_radius=model.LEVEL_SPACING, measures=("std", "entropy", "peak", "mass"))
        model.cross_check(left, right, threshold=1.0, rel=0.05)
        model.self_check(left, right, threshold=1.0, rel=0.05)
        model.refine(left, right, threshold=1.0, rel=0.05)
        model.despeckle(left, right, threshold=1.0, rel=0.05)
        model.smooth(left, right, threshold=1.0, rel=0.05)
    want = {"ecm_lr_check_fwd", "ecm_disp_splat_fwd", "ecm_disp_median_fwd", "ecm_disp_bilateral_fwd", "ecm_disp_speckle_fwd",
            "ecm_disp_wls_fwd"} | ({"ecm_eval_sparsify"} if with_distribution else set())
    assert want <= set(calls), sorted(want - set(calls))


@pytest.mark.parametrize("arch", ("cmfsm", "cmf"))
def test_bf16_inference_forward(ecm, arch):
    model, (left, right) = _model(ecm, arch).eval(), _pair()
    with recording(ecm, f"bf16:{arch}") as calls, ecm.ops.inference_dtype(torch.bfloat16), torch.no_grad():
        model(left, right)
    assert "ecm_conv3d_k3_bf16_fwd" in calls and "ecm_conv2d_bf16_fwd" in calls


def test_split_products_training_step(ecm):
    model, (left, right) = _model(ecm, "cmfsm").train(), _pair()
    with recording(ecm, "split:cmfsm") as calls, ecm.ops.split_products("bf16x3", SPLIT_ALL):
        _train_step(ecm, model, left, right, _gt())
    assert "ecm_conv3d_k3s2_split_fwd" in calls and "ecm_deconv3d_k3s2_split_fwd" in calls


def test_standalone_ops(ecm):
    ops = ecm.ops
    gen = torch.Generator(device=DEV).manual_seed(3)
    frames = torch.rand(2, 9, 14, 7, device=DEV, generator=gen) * 255.0
    rgb6 = (torch.rand(2, 9, 14, 6, device=DEV, generator=gen) * 255.0).to(torch.uint8)
    pred, gt = torch.rand(2, 9, 14, device=DEV, generator=gen) * 60.0, torch.rand(2, 9, 14, device=DEV, generator=gen) * 60.0
    with recording(ecm, "standalone") as calls:
        ops.frame_prep(frames, [1, 0], [2, 3], 6, 8, want_image=True)
        ops.frame_prep(frames, [0, 0], [0, 1], 8, 8, split=6, tail=2)
        ops.frame_prep((rgb6, frames[..., 6].half().contiguous()), [1, 0], [2, 3], 6, 8)
        ops.frame_prep_kitti_eval(frames, th=12, tw=16)
        ops.eval_epe(pred, gt, crop_h=7, crop_w=11, maxdisp=192)
        ops.eval_kitti(pred, gt, 192, per_sample=True)
        ops.disparity_to_uint16(pred, [7, 9], [14, 5])
        ops.channel_sum(torch.randn(2, 5, 3, 7, device=DEV, generator=gen))
        with pytest.raises(RuntimeError, match="invalid"):             # a window outside the frame: refused on the host, before
            ops.frame_prep(frames, [1, 0], [2, 7], 6, 8)               # any launch, and the message comes from ecm_error_string
    assert {"ecm_frame_prep", "ecm_frame_prep_packed", "ecm_frame_prep_kitti_eval", "ecm_eval_epe", "ecm_eval_kitti",
            "ecm_disp_to_u16", "ecm_channel_sum"} <= set(calls)


def test_ops_the_models_do_not_reach(ecm):
    """The rest of ops.py's entry points: the explicit cost volume, the plain regression, a 32 -> 1 convolution without the fused
    GroupNorm, the limit and mode queries, and the stateless GroupNorm entries, which ops.py takes only while its stream is being
    captured into a graph (the capture records the launches; the graph is not replayed)."""
    ops = ecm.ops
    gen = torch.Generator(device=DEV).manual_seed(4)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)                   # noqa: E731
    with recording(ecm, "others") as calls:
        ops.lr_check_max_width(), ops.disparity_splat_max_width(), ops.gn_cluster_mode(-1)
        with torch.enable_grad():
            l, r = rnd(1, 4, 5, 7).requires_grad_(), rnd(1, 4, 5, 7).requires_grad_()
            ops.cost_volume(l, r, 3).sum().backward()
            x, w = rnd(1, 8, 3, 5, 6).requires_grad_(), rnd(1, 8, 3, 3, 3).requires_grad_()
            ops.conv3d_k3(x, w, 1).sum().backward()
            ops.join_side_streams()
        ops.disparity_regression(rnd(1, 6, 5, 7))
        x, gamma, beta = rnd(1, 32, 3, 5, 6).requires_grad_(), rnd(32).requires_grad_(), rnd(32).requires_grad_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.enable_grad():             # one-time work outside the capture
            ops.group_norm_act(x, gamma, beta, relu=True).sum().backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        x.grad = gamma.grad = beta.grad = None
        with torch.cuda.graph(torch.cuda.CUDAGraph()), torch.enable_grad():
            ops.group_norm_act(x, gamma, beta, relu=True).sum().backward()
    assert {"ecm_costvol_concat_fwd", "ecm_costvol_concat_bwd", "ecm_conv3d_c1_fwd", "ecm_conv3d_c1_dgrad", "ecm_conv3d_c1_wgrad",
            "ecm_disparity_regression_fwd", "ecm_gn3d_fwd", "ecm_gn3d_bwd"} <= set(calls)


def test_gn3d_apply_from_a_host(ecm):
    """ecm_gn3d_apply has no caller in the package (ABI_ONLY): the two-stage pair as a host of the C ABI would call it, through the
    same prototypes, against torch's GroupNorm in fp64.  Operands of unit scale, 2 x 64 x 210: the statistics and the affine step
    round a handful of times in fp32 (2^-24 relative each) on values below 8, so 1e-5 is two orders above the expected error."""
    lib = ecm._lib
    gen = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(2, 64, 5, 6, 7, device=DEV, generator=gen)
    gamma, beta = torch.randn(64, device=DEV, generator=gen), torch.randn(64, device=DEV, generator=gen)
    y, stats = torch.empty_like(x), torch.empty(2, 32, 2, device=DEV)
    S, p, st = 5 * 6 * 7, (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = lib.query("ecm_gn3d_scratch_bytes", 2, 64, C.c_longlong(S))
    scratch = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    lib.call("ecm_gn3d_stats", p(x), p(stats), p(scratch), C.c_longlong(nb), 2, 64, C.c_longlong(S), 1e-5, st)
    lib.call("ecm_gn3d_apply", p(x), p(stats), p(gamma), p(beta), None, p(y), 2, 64, C.c_longlong(S), 1, st)
    ecm.ops.check_async_errors()
    want = torch.relu(torch.nn.functional.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5))
    assert float((y.double() - want).abs().max()) <= 1e-5


def test_every_prototype_was_called_or_is_accounted_for(ecm):
    """Runs last: reads what the cases above recorded; runs no model."""
    expected = {f"train:{a}" for a in ARCHS} | {f"infer:{a}" for a in ARCHS} | {"bf16:cmfsm", "bf16:cmf", "split:cmfsm", "standalone", "others"}
    assert CASES == expected, f"run the whole module: the cases {sorted(expected - CASES)} did not record"
    for name, (v, i) in sorted(INT_MAX.items(), key=lambda kv: -kv[1][0]):             # what DESIGN.md's headroom note scales up
        print(f"largest int argument at {H}x{W}, batch 1: {name} argument {i} = {v}")
    table = set(ecm._lib.PROTOTYPES)
    unknown, both, missing = sorted(RECORDED - table), sorted(RECORDED & set(ABI_ONLY)), sorted(table - RECORDED - set(ABI_ONLY))
    assert not (unknown or both or missing), (f"recorded but not in PROTOTYPES: {unknown}; called by the package, so not ABI-only: "
                                              f"{both}; neither recorded nor in ABI_ONLY ({len(missing)}): {missing}")
    assert RECORDED | set(ABI_ONLY) == table
