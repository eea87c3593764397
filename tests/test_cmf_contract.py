"""CPU contract of the `cmf` architecture (cmf/models/cmf.py): registry entry, parameter tree, input checks, and the 2-D
kernel family's instantiation table that its decoder needs.  No GPU."""
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def ecm():
    import ecm_amd
    return ecm_amd


@pytest.fixture(scope="module")
def model(ecm):
    m = ecm.get_model("cmf")
    assert m is not None, "get_model('cmf') must return the cmf architecture"
    return m


def test_registry_serves_cmf(ecm, model):
    assert isinstance(model, ecm.models.cmf) and isinstance(model, ecm.cmf)
    assert model.maxdisp == 192


def test_state_dict_matches_reference(model):
    with open(os.path.join(GOLDEN, "cmf_state_shapes.json")) as f:
        ref = json.load(f)
    sd = model.state_dict()
    assert list(sd) == list(ref), "state_dict keys (and their order) must be the reference's"
    bad = [k for k, v in ref.items() if list(sd[k].shape) != v]
    assert not bad, bad
    # the reference checkpoint's decoder biases are present
    for k in ("srr.deconv_module_list.0.0.bias", "srr.deconv_module_list.1.0.bias", "srr.conv_out.bias"):
        assert k in sd


def test_reference_state_dict_loads(model):
    from oracle.weights import make_state_dict
    with open(os.path.join(GOLDEN, "cmf_state_shapes.json")) as f:
        ref = json.load(f)
    model.load_state_dict(make_state_dict(ref))           # strict


def test_every_layer_is_native(ecm, model):
    """No layer of cmf may need the vendor-library fallback: every Conv2d is inside the native 2-D family, the decoder's
    transposed convolutions and conv_out have their own kernels."""
    M, ops = ecm.models, ecm.ops
    n_enc = n_dec = 0
    for name, m in model.named_modules():
        if isinstance(m, M.HipConv2dC1):
            assert m._native(), name
            n_dec += 1
        elif isinstance(m, M.EncConv2d):
            assert m._native(), name
            n_enc += 1
        elif isinstance(m, M.HipConvTranspose2d):
            assert m._native(), name
            n_dec += 1
        elif isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            assert name.startswith("mapping_matrix"), f"{name}: a plain nn layer in cmf"
    assert n_dec == 3 and n_enc > 40, (n_dec, n_enc)
    # the decoder's deconv data gradient: a stride-2 3x3 Conv2d 64 -> 96 (COT-3)
    assert ops.conv2d_supported(64, 96, 3, 3, 2, 1)


def test_cot3_stride2_instantiation_matches_table(ecm):
    """_C2_CASES mirrors the COTS masks of csrc/conv2d_case_*.hip; the stride-2 3x3 case now includes COT 3."""
    src = open(os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd", "csrc", "conv2d_case_k33_s2_d1.hip")).read()
    mask = int(re.search(r"dispatch_c2<3, 3, 2, 1, (\d+)>", src).group(1))
    cots = {c for c in range(1, 5) if mask & (1 << c)}
    assert cots == ecm.ops._C2_CASES[(3, 3, 2, 1)] == {1, 2, 3, 4}


@pytest.mark.parametrize("hw", [(250, 512), (256, 510), (258, 514)])
def test_size_not_multiple_of_4_is_refused(model, hw):
    """Refused with a ValueError that names the constraint BEFORE any kernel runs (the inputs are CPU tensors: any op would
    raise a RuntimeError instead)."""
    x = torch.zeros(1, 3, *hw)
    with pytest.raises(ValueError, match="multiples of 4"):
        model(x, x)


def test_decoder_refuses_mismatched_maps(ecm):
    srr = ecm.super_resolution_refinement(32, 2)
    preds = torch.zeros(3, 1, 8, 16)
    with pytest.raises(ValueError):
        srr(preds, torch.zeros(1, 3, 32, 64), torch.zeros(1, 32, 8, 16), torch.zeros(1, 32, 16, 30))


def test_cpu_tensors_do_not_fall_back(model):
    """A valid size on CPU tensors reaches the native ops, which refuse CPU tensors: no silent eager path."""
    x = torch.zeros(1, 3, 64, 128)
    with pytest.raises(RuntimeError):
        model(x, x)
