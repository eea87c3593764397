"""CPU-side contract of the opt-in bf16 encoder (ops.encoder_dtype): the switch itself, the inference-only guard (it raises
before anything reaches the device), and the new C ABI entries.  No GPU needed."""
import os

import pytest
import torch

from test_abi_types import declared

NEW_ENTRIES = ("ecm_conv2d_bf16_packed_elems", "ecm_conv2d_bf16_pack_weight", "ecm_conv2d_bf16_fwd", "ecm_gn3d_apply_bf16_f32")


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
    assert not ecm.ops.encoder_bf16()


def test_encoder_dtype_nests_and_restores(ecm):
    ops = ecm.ops
    with ops.encoder_dtype(torch.bfloat16):
        assert ops.encoder_bf16()
        with ops.encoder_dtype(torch.float32):
            assert not ops.encoder_bf16()
            with ops.encoder_dtype(torch.bfloat16):
                assert ops.encoder_bf16()
            assert not ops.encoder_bf16()
        assert ops.encoder_bf16()
    assert not ops.encoder_bf16()


def test_encoder_dtype_restores_on_exception(ecm):
    ops = ecm.ops
    with pytest.raises(KeyError):
        with ops.encoder_dtype(torch.bfloat16):
            raise KeyError("boom")
    assert not ops.encoder_bf16()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64, torch.int32])
def test_encoder_dtype_rejects_other_dtypes(ecm, dtype):
    with pytest.raises(ValueError):
        with ecm.ops.encoder_dtype(dtype):
            pass
    assert not ecm.ops.encoder_bf16()


def test_independent_of_aggregation_dtype(ecm):
    ops = ecm.ops
    with ops.encoder_dtype(torch.bfloat16):
        assert ops.encoder_bf16() and not ops.aggregation_bf16()
        with ops.aggregation_dtype(torch.bfloat16):
            assert ops.encoder_bf16() and ops.aggregation_bf16()
            with ops.encoder_dtype(torch.float32):
                assert not ops.encoder_bf16() and ops.aggregation_bf16()
        assert ops.encoder_bf16() and not ops.aggregation_bf16()
    with ops.aggregation_dtype(torch.bfloat16):
        assert ops.aggregation_bf16() and not ops.encoder_bf16()
    assert not ops.encoder_bf16() and not ops.aggregation_bf16()


@pytest.mark.parametrize("variant", ["cmfsm", "sub8", "cmf"])
def test_grad_enabled_encoder_raises_before_any_launch(ecm, variant):
    """CPU tensors: any launch attempt would raise the CPU-tensor error instead of the inference-only one."""
    fe = ecm.models.feature_extraction(variant)
    x = torch.zeros(2, 3, 32, 64)
    with ecm.ops.encoder_dtype(torch.bfloat16):
        with pytest.raises(RuntimeError, match="no backward"):
            fe(x)
    with pytest.raises(RuntimeError, match="CPU tensor"):       # outside the block: the fp32 path's own error
        fe(x)


def test_bf16_conv_with_grad_raises(ecm):
    with pytest.raises(RuntimeError, match="no backward"):
        ecm.ops.conv2d_bf16(torch.zeros(1, 32, 4, 8, dtype=torch.bfloat16), torch.zeros(32, 32, 3, 3))


def test_no_grad_bf16_conv_still_refuses_cpu(ecm):
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA"):
            ecm.ops.conv2d_bf16(torch.zeros(1, 32, 4, 8, dtype=torch.bfloat16), torch.zeros(32, 32, 3, 3))


def test_coverage_of_every_encoder_layer(ecm):
    """Every EncConv2d after the stem of all five encoder variants is inside the bf16 kernel's coverage."""
    sup = ecm.ops.conv2d_bf16_supported
    for variant in ("cmfsm", "sub4", "sub8", "sub16", "cmf"):
        fe = ecm.models.feature_extraction(variant)
        convs = [m for m in fe.modules() if isinstance(m, ecm.models.EncConv2d)]
        stem = fe.firstconv[0][0]
        for m in convs:
            if m is stem:
                assert m.in_channels == 3
                continue
            assert m._native_bf16(), (variant, m)
    assert not sup(3, 32, 3, 1, 1) and not sup(32, 48, 3, 1, 1) and not sup(32, 32, 3, 2, 2) and not sup(32, 32, 5, 1, 1)


def test_new_entries_exported_and_prototyped(lib_mod):
    import ctypes
    lib = ctypes.CDLL(lib_mod.LIB_PATH)
    for n in NEW_ENTRIES:
        assert n in lib_mod.PROTOTYPES, n
        assert hasattr(lib, n), n
        assert n in declared(), n


def test_pack_size_query_and_null_checks(lib_mod):
    import ctypes
    assert lib_mod.query("ecm_conv2d_bf16_packed_elems", 32, 64, 3) == 32 * 9 * 64
    assert lib_mod.query("ecm_conv2d_bf16_packed_elems", 128, 32, 1) == 128 * 32
    assert lib_mod.query("ecm_conv2d_bf16_packed_elems", 24, 32, 3) == 0          # Ci % 16 != 0
    assert lib_mod.query("ecm_conv2d_bf16_packed_elems", 32, 32, 5) == 0          # k not 1 or 3
    lib = lib_mod.load()
    assert lib.ecm_conv2d_bf16_fwd(None, None, None, 1, 32, 32, 8, 8, 3, 1, 1, 0, None) == -1
    assert lib.ecm_gn3d_apply_bf16_f32(None, None, None, None, None, None, None, 1, 32, ctypes.c_longlong(8), 0, None) == -1
