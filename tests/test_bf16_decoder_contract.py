"""CPU-side contract of the opt-in bf16 decoder (ops.decoder_dtype, ops.inference_dtype): the switch itself, the
inference-only guard (it raises before anything reaches the device), the layer coverage and the new C ABI entries.
No GPU needed."""
import itertools
import os

import pytest
import torch

from test_abi_types import declared

BF = torch.bfloat16
NEW_ENTRIES = ("ecm_deconv2d_bf16_packed_elems", "ecm_deconv2d_bf16_pack_weight", "ecm_deconv2d_k3s2_bias_bf16_fwd",
               "ecm_conv2d_c1_bf16_fwd")


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
    assert not ecm.ops.decoder_bf16()


def test_decoder_dtype_nests_and_restores(ecm):
    ops = ecm.ops
    with ops.decoder_dtype(BF):
        assert ops.decoder_bf16()
        with ops.decoder_dtype(torch.float32):
            assert not ops.decoder_bf16()
            with ops.decoder_dtype(BF):
                assert ops.decoder_bf16()
            assert not ops.decoder_bf16()
        assert ops.decoder_bf16()
    assert not ops.decoder_bf16()


def test_decoder_dtype_restores_on_exception(ecm):
    ops = ecm.ops
    with pytest.raises(KeyError):
        with ops.decoder_dtype(BF):
            raise KeyError("boom")
    assert not ops.decoder_bf16()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64, torch.int32])
def test_rejects_other_dtypes(ecm, dtype):
    for scope in (ecm.ops.decoder_dtype, ecm.ops.inference_dtype):
        with pytest.raises(ValueError):
            with scope(dtype):
                pass
    assert not (ecm.ops.decoder_bf16() or ecm.ops.encoder_bf16() or ecm.ops.aggregation_bf16())


@pytest.mark.parametrize("enc,agg,dec", list(itertools.product([False, True], repeat=3)))
def test_three_switches_are_independent(ecm, enc, agg, dec):
    ops = ecm.ops
    dt = lambda on: BF if on else torch.float32
    with ops.encoder_dtype(dt(enc)), ops.aggregation_dtype(dt(agg)), ops.decoder_dtype(dt(dec)):
        assert (ops.encoder_bf16(), ops.aggregation_bf16(), ops.decoder_bf16()) == (enc, agg, dec)
        with ops.decoder_dtype(dt(not dec)):                 # flipping one leaves the other two alone
            assert (ops.encoder_bf16(), ops.aggregation_bf16(), ops.decoder_bf16()) == (enc, agg, not dec)
        assert (ops.encoder_bf16(), ops.aggregation_bf16(), ops.decoder_bf16()) == (enc, agg, dec)
    assert (ops.encoder_bf16(), ops.aggregation_bf16(), ops.decoder_bf16()) == (False, False, False)


def test_inference_dtype_sets_and_restores_all_three(ecm):
    ops = ecm.ops
    state = lambda: (ops.encoder_bf16(), ops.aggregation_bf16(), ops.decoder_bf16())
    with ops.inference_dtype(BF):
        assert state() == (True, True, True)
        with ops.inference_dtype(torch.float32):
            assert state() == (False, False, False)
        assert state() == (True, True, True)
    assert state() == (False, False, False)
    with ops.encoder_dtype(BF):                              # it restores what was there, not the default
        with ops.inference_dtype(BF):
            assert state() == (True, True, True)
        assert state() == (True, False, False)
    with pytest.raises(KeyError):
        with ops.inference_dtype(BF):
            raise KeyError("boom")
    assert state() == (False, False, False)


def _decoder_inputs(B=1, h=4, w=8):
    return (torch.zeros(3, B, h, w), torch.zeros(B, 3, 4 * h, 4 * w), torch.zeros(B, 32, h, w), torch.zeros(B, 32, 2 * h, 2 * w))


def test_grad_enabled_decoder_raises_before_any_launch(ecm):
    """CPU tensors: any launch attempt would raise the CPU-tensor error instead of the inference-only one."""
    srr = ecm.models.super_resolution_refinement(32, 2)
    ins = _decoder_inputs()
    with ecm.ops.decoder_dtype(BF):
        with pytest.raises(RuntimeError, match="no backward"):
            srr(*ins)
    with pytest.raises(RuntimeError, match="CPU tensor"):       # outside the block: the fp32 path's own error
        srr(*ins)


def test_grad_enabled_cmf_raises_before_any_launch(ecm):
    model = ecm.get_model("cmf")
    x = torch.zeros(1, 3, 64, 128)
    with ecm.ops.decoder_dtype(BF):
        with pytest.raises(RuntimeError, match="no backward"):
            model(x, x)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        model(x, x)


def test_new_ops_with_grad_raise(ecm):
    ops = ecm.ops
    with pytest.raises(RuntimeError, match="no backward"):
        ops.deconv2d_k3s2_bias_bf16(torch.zeros(1, 96, 4, 8, dtype=BF), torch.zeros(96, 64, 3, 3), torch.zeros(64))
    with pytest.raises(RuntimeError, match="no backward"):
        ops.conv2d_c1_relu_bf16(torch.zeros(1, 96, 4, 8, dtype=BF), torch.zeros(1, 96, 3, 3), torch.zeros(1))


def test_no_grad_new_ops_still_refuse_cpu(ecm):
    ops = ecm.ops
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA"):
            ops.deconv2d_k3s2_bias_bf16(torch.zeros(1, 96, 4, 8, dtype=BF), torch.zeros(96, 64, 3, 3), torch.zeros(64))
        with pytest.raises(RuntimeError, match="CUDA"):
            ops.conv2d_c1_relu_bf16(torch.zeros(1, 96, 4, 8, dtype=BF), torch.zeros(1, 96, 3, 3), torch.zeros(1))


def test_coverage_of_every_decoder_layer(ecm):
    """Every layer of the decoder after the two fp32 stems (conv1 1 -> 64, rgb_fea 3 -> 32) is inside a bf16 kernel."""
    ops, models = ecm.ops, ecm.models
    assert ops.conv2d_bf16_supported(96, 96, 3, 1, 1) and ops.conv2d_bf16_supported(32, 32, 3, 1, 1)
    assert ops.deconv2d_bf16_supported(96, 64) and ops.deconv2d_bf16_supported(32, 32)
    assert not ops.deconv2d_bf16_supported(24, 64) and not ops.deconv2d_bf16_supported(96, 48)
    srr = models.super_resolution_refinement(32, 2)
    stems = (srr.conv1[0][0], srr.rgb_fea[0][0])
    assert [m.in_channels for m in stems] == [1, 3]
    for m in srr.modules():
        if isinstance(m, models.EncConv2d) and not any(m is s for s in stems):
            assert m._native_bf16(), m
        elif isinstance(m, models.HipConvTranspose2d):
            assert m._native() and ops.deconv2d_bf16_supported(m.in_channels, m.out_channels), m
        elif isinstance(m, models.HipConv2dC1):
            assert m._native() and m.in_channels % 16 == 0, m


def test_new_entries_exported_and_prototyped(lib_mod):
    import ctypes
    lib = ctypes.CDLL(lib_mod.LIB_PATH)
    for n in NEW_ENTRIES:
        assert n in lib_mod.PROTOTYPES, n
        assert hasattr(lib, n), n
        assert n in declared(), n
    assert lib_mod.query("ecm_abi_version") >= 5


def test_pack_size_query_and_null_checks(lib_mod):
    assert lib_mod.query("ecm_deconv2d_bf16_packed_elems", 96, 64) == 96 * 9 * 64
    assert lib_mod.query("ecm_deconv2d_bf16_packed_elems", 32, 32) == 32 * 9 * 32
    assert lib_mod.query("ecm_deconv2d_bf16_packed_elems", 24, 64) == 0           # Ci % 16 != 0
    assert lib_mod.query("ecm_deconv2d_bf16_packed_elems", 96, 48) == 0           # Co not 32 or 64
    lib = lib_mod.load()
    assert lib.ecm_deconv2d_bf16_pack_weight(None, None, 96, 64, None) == -1
    assert lib.ecm_deconv2d_k3s2_bias_bf16_fwd(None, None, None, None, 1, 96, 64, 8, 8, None) == -1
    assert lib.ecm_conv2d_c1_bf16_fwd(None, None, None, None, 1, 96, 8, 8, None) == -1
