"""CPU-side contract of the opt-in bf16 aggregation (ops.aggregation_dtype): the switch itself, the inference-only guard (it
raises before anything reaches the device), and the new C ABI entries.  No GPU needed."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_abi_types import declared

NEW_ENTRIES = ("ecm_conv3d_bf16_packed_elems", "ecm_conv3d_bf16_pack_weight", "ecm_conv3d_k3_bf16_fwd",
               "ecm_deconv3d_k3s2_bf16_fwd", "ecm_gn3d_stats_bf16", "ecm_gn3d_apply_bf16", "ecm_gn3d_apply_f32_bf16",
               "ecm_conv3d_c1_gn_fwd_bf16")


@pytest.fixture(scope="module")
def ecm():
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def lib_mod(ecm):
    if not os.path.exists(ecm._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm._lib


def test_default_is_fp32(ecm):
    assert not ecm.ops.aggregation_bf16()


def test_aggregation_dtype_nests_and_restores(ecm):
    ops = ecm.ops
    with ops.aggregation_dtype(torch.bfloat16):
        assert ops.aggregation_bf16()
        with ops.aggregation_dtype(torch.float32):
            assert not ops.aggregation_bf16()
            with ops.aggregation_dtype(torch.bfloat16):
                assert ops.aggregation_bf16()
            assert not ops.aggregation_bf16()
        assert ops.aggregation_bf16()
    assert not ops.aggregation_bf16()


def test_aggregation_dtype_restores_on_exception(ecm):
    ops = ecm.ops
    with pytest.raises(KeyError):
        with ops.aggregation_dtype(torch.bfloat16):
            raise KeyError("boom")
    assert not ops.aggregation_bf16()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64, torch.int32])
def test_aggregation_dtype_rejects_other_dtypes(ecm, dtype):
    with pytest.raises(ValueError):
        with ecm.ops.aggregation_dtype(dtype):
            pass
    assert not ecm.ops.aggregation_bf16()


def test_grad_enabled_3d_op_raises_inside_block(ecm):
    """A 3-D op inside the block with grad enabled raises the inference-only error -- before the device is touched (these are
    CPU tensors: any launch attempt would raise a different error)."""
    ops = ecm.ops
    x, w = torch.zeros(1, 32, 2, 2, 4), torch.zeros(32, 32, 3, 3, 3)
    g, b = torch.ones(32), torch.zeros(32)
    with ops.aggregation_dtype(torch.bfloat16):
        for fn in (lambda: ops.conv3d_k3(x, w), lambda: ops.deconv3d_k3s2(x, w),
                   lambda: ops.classifier_tail(x, g, b, torch.zeros(1, 32, 3, 3, 3)),
                   lambda: ops.costvol_conv3d(torch.zeros(1, 32, 2, 4), torch.zeros(1, 32, 2, 4), torch.zeros(32, 64, 3, 3, 3), 4)):
            with pytest.raises(RuntimeError, match="no backward"):
                fn()


def test_bf16_volume_with_grad_raises(ecm):
    ops = ecm.ops
    x = torch.zeros(1, 32, 2, 2, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.conv3d_k3(x, torch.zeros(32, 32, 3, 3, 3))
    with pytest.raises(RuntimeError, match="no backward"):
        ops.group_norm_act(x, torch.ones(32), torch.zeros(32))


@pytest.mark.parametrize("shape", [(1, 32, 4, 4), (1, 32, 4, 2, 2)])
def test_encoder_group_norm_is_not_guarded(ecm, shape):
    """An fp32 GroupNorm is not guarded: the encoder's (also on 5-D phase planes of its dilated stages) runs before the 3-D
    stack and reaches the usual fp32 checks (CPU tensor error); the stack's first GroupNorm follows a guarded op."""
    ops = ecm.ops
    with ops.aggregation_dtype(torch.bfloat16):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.group_norm_act(torch.zeros(*shape), torch.ones(32), torch.zeros(32))


def test_no_grad_bf16_op_still_refuses_cpu(ecm):
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA"):
            ecm.ops.conv3d_k3(torch.zeros(1, 32, 2, 2, 4, dtype=torch.bfloat16), torch.zeros(32, 32, 3, 3, 3))


def test_new_entries_exported_and_prototyped(lib_mod):
    import ctypes
    lib = ctypes.CDLL(lib_mod.LIB_PATH)
    for n in NEW_ENTRIES:
        assert n in lib_mod.PROTOTYPES, n
        assert hasattr(lib, n), n
    assert all(n in declared() for n in NEW_ENTRIES)


def test_bf16_size_query_and_null_checks(lib_mod):
    assert lib_mod.query("ecm_conv3d_bf16_packed_elems", 32, 64) == 4 * 28 * 64 * 8
    assert lib_mod.query("ecm_conv3d_bf16_packed_elems", 12, 32) == 0            # Ci % 8 != 0
    lib = lib_mod.load()
    assert lib.ecm_conv3d_k3_bf16_fwd(None, None, None, 1, 32, 32, 4, 4, 4, 1, None) == -1
    assert lib.ecm_deconv3d_k3s2_bf16_fwd(None, None, None, 1, 64, 32, 4, 4, 4, None) == -1
    assert lib.ecm_gn3d_apply_bf16(None, None, None, None, None, None, 1, 32, ctypes_ll(8), 0, None) == -1


def ctypes_ll(v):
    import ctypes
    return ctypes.c_longlong(v)


def test_private_segment_audit_on_rebuilt_library(lib_mod):
    """The new kernels keep the library free of private segments (tools/check_private_segment.py over every kernel)."""
    so = lib_mod.LIB_PATH
    tools = ("/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objcopy", "/opt/rocm/lib/llvm/bin/clang-offload-bundler")
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("needs the ROCm llvm binutils")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_private_segment.py"), so], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 with a private segment" in r.stdout
    assert "conv3d_bf16" in r.stdout or "kernels audited" in r.stdout
