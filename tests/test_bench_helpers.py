"""CPU checks of bench.py's bookkeeping helpers (no GPU, no library): the kernel-family table of `step_breakdown_ms` / the launch
table, and the argument parser's defaults the driver relies on (`python bench.py` with no flags = one GPU, a few steps)."""
import importlib.util
import os
import sys

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("ecm_bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_kernel_families():
    b = _bench()
    f = b._family
    assert f("ecm_conv_wino_fwd", (4, 32, 32, 48, 144, 240, 3)) == "winograd_conv_3d"
    assert f("ecm_conv_wino_fwd_add", (8, 64, 64, 1, 144, 240, 1)) == "winograd_conv_2d"
    assert f("ecm_conv_wino_wgrad", (4, 32, 32, 48, 144, 240, 3)) == "winograd_wgrad_3d"       # the scratch size rides in .longs, not here
    assert f("ecm_conv_wino_wgrad", (8, 64, 64, 1, 144, 240, 1)) == "winograd_wgrad_2d"
    assert f("ecm_conv3d_k3_fwd", (4, 32, 64, 48, 144, 240, 2)) == "stride2_conv_deconv_wgrad_3d"
    assert f("ecm_conv3d_k3_wgrad", (4, 32, 32, 48, 144, 240, 1)) == "direct_conv_3d_stride1"
    assert f("ecm_deconv3d_k3s2_fwd", (4, 64, 32, 24, 72, 120, 48, 144, 240)) == "stride2_conv_deconv_wgrad_3d"
    assert f("ecm_gn3d_bwd_p", (4, 32, 1)) == "groupnorm" and f("ecm_gn3d_stats", (4, 32)) == "groupnorm"
    assert f("ecm_conv3d_c1_gn_fwd", (4, 32, 48, 144, 240)) == "classifier_32to1"
    assert f("ecm_weights9_bwd", (4, 144, 240, 4)) == "ecm_weights"
    assert f("ecm_conv2d_fwd_ex", (8, 3, 32)) == "conv2d_direct_family"
    assert f("ecm_conv_wino_pack_weight2", (32, 32, 3)) == "weight_packing"
    assert f("ecm_costvol_conv_assemble_fwd", (4, 32, 48, 144, 240)) == "cost_volume_assemble"
    assert f("ecm_stereo_loss_fwd", ()) == "heads_and_loss" and f("ecm_sum_n", ()) == "gradient_sums"
    assert f("ecm_something_new", (1,)) == "other_hip"


def test_default_arguments_are_the_single_gpu_headline(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = b.parse()
    assert a.gpus == 1 and a.mode == "train" and (a.batch, a.height, a.width, a.maxdisp) == (4, 576, 960, 192)
    assert 1 <= a.steps <= 20 and 1 <= a.warmup <= 5              # finishes within minutes with no flags
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "50", "--warmup", "10"])
    a = b.parse()
    assert (a.gpus, a.steps, a.warmup) == (8, 50, 10)


def test_plain_run_and_full_options(monkeypatch):
    """A plain run measures the headline only; --full turns the rest on; --steps really is the number of timed steps."""
    import pytest
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    a = b.parse()
    assert a.steps == 7 and not a.full and a.dump_outputs == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out", "--launch-table", "t.json"])
    a = b.parse()
    assert a.full and a.dump_outputs == "out" and a.launch_table == "t.json"
    for argv in (["bench.py", "--steps", "0"], ["bench.py", "--launch-table", "t.json"]):
        monkeypatch.setattr(sys, "argv", argv)
        with pytest.raises(SystemExit):
            b.parse()


def test_dump_outputs_fit_the_budget_and_repeat(tmp_path):
    """--dump-outputs at the default geometry: the small arrays whole, the gradient and parameter vectors as a fixed sample,
    float32, at most 64 MB in all, and the same elements in every run."""
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(3)
    outs = {"loss": torch.tensor(0.25), **{f"disp{i}": torch.rand(4, 576, 960, generator=g) for i in (1, 2, 3)},
            "grads": torch.randn(5255368, generator=g), "params": torch.randn(5255368, generator=g)}
    written = b.dump_outputs(outs, str(tmp_path / "a"))
    b.dump_outputs(outs, str(tmp_path / "b"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64e6
    for k, t in outs.items():
        x, y = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y) and x.size == written[k]
        if k.startswith("disp") or k == "loss":
            assert np.array_equal(x, t.numpy())
        else:
            assert 0 < x.size < t.numel() and np.isin(x, t.numpy()).all()
    assert b.dump_budget({"a": 10, "b": 100, "c": 100}, 110) == {"a": 10, "b": 50, "c": 50}
