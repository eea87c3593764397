"""What the frame decodes share: the refusals of ops.frame_prep / ops.frame_prep_kitti_eval that come before
any library call -- window origins that are not one per sample, a mean or std that is not three finite numbers, a shard with a
tensor off the device (one GPU cannot show two devices: the equal-device condition itself is not exercised) -- and the chunk
boundary of the origin copy of csrc/frame_io.h: a batch one past the 32 samples (64 views) that one launch carries origins for
equals, bit for bit, its samples decoded one by one."""
import random

import numpy as np
import pytest
import torch

from frame_fixtures import float_frames, packed_shard
from test_hip_abi_calls import recording

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available(), "needs the MI355X"
    import ecm_amd
    return ecm_amd


def test_refusals_come_before_any_library_call(ecm):
    ops = ecm.ops
    rgb, dsp, frames = float_frames(2, 8, 9, 1)
    on_dev, shard, split_shard = frames.cuda(), (rgb.cuda(), dsp.cuda()), (rgb.cuda(), dsp)
    nan = float("nan")
    with recording(ecm, "frame decode refusals", census=False) as calls:
        for f in (on_dev, shard):
            for ys, xs in (([0], [0, 0]), ([0, 0], [0]), ([0, 0, 0], [0, 0]), ([0, 0], [0, 0, 0]), ([0], [0]), ([0, 0, 0], [0, 0, 0])):
                with pytest.raises(ValueError, match="one window origin per sample"):
                    ops.frame_prep(f, ys, xs, 4, 5)
            for kw in (dict(mean=(0.5, 0.5)), dict(std=(0.2, nan, 0.2)), dict(mean=(0.5, 0.5, 0.5, 0.5)), dict(std=(0.2, float("inf"), 0.2))):
                with pytest.raises(ValueError, match="three finite numbers"):
                    ops.frame_prep(f, [0, 0], [0, 0], 4, 5, **kw)
                with pytest.raises(ValueError, match="three finite numbers"):
                    ops.frame_prep_kitti_eval(f, th=12, tw=16, **kw)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.frame_prep(split_shard, [0, 0], [0, 0], 4, 5)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.frame_prep_kitti_eval(split_shard, th=12, tw=16)
        with pytest.raises(ValueError, match="one window origin per sample"):
            ops.frame_prep_jitter(shard, [0], [0, 0], 4, 5, ops.jitter_params(2, random.Random(0), torch.Generator()))
        assert not [c for c in calls if "frame_prep" in c], calls
        ops.check_async_errors()
    assert calls and not [c for c in calls if "frame_prep" in c], calls        # only the status query went to the library
    with recording(ecm, "frame decode accepted", census=False) as calls:       # and the recorder does see a decode that is taken
        ops.frame_prep(on_dev, [0, 4], [4, 0], 4, 5)
        ops.frame_prep(shard, [0, 4], [4, 0], 4, 5)
        ops.frame_prep_kitti_eval(shard, th=12, tw=16)
        as_tuples = ops.frame_prep(shard, [0, 4], [4, 0], 4, 5, mean=(0.5, 0.25, 0.125), std=(0.5, 2.0, 4.0))
        as_arrays = ops.frame_prep(shard, [0, 4], [4, 0], 4, 5, mean=torch.tensor([0.5, 0.25, 0.125]), std=np.array([0.5, 2.0, 4.0], np.float32))
    assert {"ecm_frame_prep", "ecm_frame_prep_packed"} <= set(calls)
    assert all(torch.equal(a, b) for a, b in zip(as_tuples, as_arrays))         # any sequence of three finite numbers is a mean or std


B33, H33, W33, TH33, TW33 = 33, 6, 9, 4, 5                                     # one past FP_MAXB: views 64 and 65 of the jitter's chunk
ORIGINS = [b % (H33 - TH33 + 1) for b in range(B33)], [b % (W33 - TW33 + 1) for b in range(B33)]


def one_by_one(decode, B):
    """The concatenation of `decode(b)` (a batch of one) over the samples."""
    outs = [decode(b) for b in range(B)]
    return [torch.cat([o[k] for o in outs]) for k in range(len(outs[0]))]


@pytest.mark.parametrize("form", ["float32", "packed fp16", "packed fp32"])
def test_frame_prep_across_the_chunk_boundary_is_its_samples_one_by_one(ecm, form):
    ys, xs = ORIGINS
    # the frame admits 15 origins, so those of 33 samples repeat with period 15: all are used, neighbours differ, and sample 32 differs
    # from sample 0, the one whose origin it would take if the second chunk read the first chunk's slots
    assert len(set(zip(ys, xs))) == 15 and (ys[32], xs[32]) != (ys[0], xs[0]) and (ys[32], xs[32]) != (ys[31], xs[31])
    rgb, dsp, frames = float_frames(B33, H33, W33, 2)
    src = (frames.cuda(),) if form == "float32" else (rgb.cuda(), (dsp.half() if form == "packed fp16" else dsp).cuda())
    take = (lambda b: src[0][b:b + 1]) if form == "float32" else (lambda b: (src[0][b:b + 1], src[1][b:b + 1]))          # noqa: E731
    whole = ecm.ops.frame_prep(src[0] if form == "float32" else src, ys, xs, TH33, TW33, want_image=True)
    parts = one_by_one(lambda b: ecm.ops.frame_prep(take(b), ys[b:b + 1], xs[b:b + 1], TH33, TW33, want_image=True), B33)
    assert len(whole) == 4 and all(torch.equal(w, p) for w, p in zip(whole, parts))
    for b in (0, 31, 32):                                                      # and the window is the one asked for
        assert torch.equal(whole[3][b].cpu(), rgb[b, ys[b]:ys[b] + TH33, xs[b]:xs[b] + TW33, :3].permute(2, 0, 1).float())
    ecm.ops.check_async_errors()


@pytest.mark.parametrize("half", [True, False])
def test_frame_prep_jitter_across_the_chunk_boundary_is_its_samples_one_by_one(ecm, half):
    ops = ecm.ops
    ys, xs = ORIGINS
    rgb, dsp = (t.cuda() for t in packed_shard(B33, H33, W33, half, 3))
    p = ops.jitter_params(B33, random.Random(7), torch.Generator().manual_seed(8))
    assert bool((p.order[32] == 1).any(-1).all()) and bool((p.order[0] == 1).any(-1).all())       # contrast in the last sample's views
    whole = ops.frame_prep_jitter((rgb, dsp), ys, xs, TH33, TW33, p, want_image=True)
    one = lambda b: ops.JitterParams(p.factors[b:b + 1], p.order[b:b + 1], p.hue_shift[b:b + 1], p.pca[b:b + 1])      # noqa: E731
    parts = one_by_one(lambda b: ops.frame_prep_jitter((rgb[b:b + 1], dsp[b:b + 1]), ys[b:b + 1], xs[b:b + 1], TH33, TW33, one(b),
                                                       want_image=True), B33)
    assert len(whole) == 4 and all(torch.equal(w, q) for w, q in zip(whole, parts))
    assert torch.equal(whole[2][32].cpu(), dsp[32, ys[32]:ys[32] + TH33, xs[32]:xs[32] + TW33].float().cpu())
    ops.check_async_errors()
