"""What the tests of the three frame decodes share (ops.frame_prep, ops.frame_prep_jitter, ops.remap_pair):
seeded random frames in the forms the decodes take, and the loader's normalisation statements in fp32 on the CPU.  Not a test module.

Every frame comes from packed_shard, so a packed shard, its float32 [B,H,W,7] frame and its raw left view hold the same bytes."""
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                     # cmf/loader/Flying3d.py:26-27


def packed_shard(B, H, W, half, seed):
    """(rgb6 uint8 [B,H,W,6], disparity fp16|fp32 [B,H,W] in 0..200) on the host."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (B, H, W, 6), dtype=torch.uint8, generator=g)
    dsp = torch.rand(B, H, W, generator=g) * 200
    return rgb, (dsp.half() if half else dsp)


def float_frames(B, H, W, seed):
    """(rgb6, disparity fp32, frames): the shard and the float32 [B,H,W,7] frame the reference stores for it (flying3ddata.py:34-39:
    uint8 images promoted to float32, the disparity behind them)."""
    rgb, dsp = packed_shard(B, H, W, False, seed)
    return rgb, dsp, torch.cat([rgb.float(), dsp.unsqueeze(-1)], -1).contiguous()


def raw_views(B, H, W, seed, kind="u8"):
    """The shard's left view as remap_pair takes a raw frame: uint8 [B,H,W,3], or float32 [B,3,H,W] holding the same 0..255."""
    raw = packed_shard(B, H, W, False, seed)[0][..., :3].contiguous()
    return raw if kind == "u8" else raw.permute(0, 3, 1, 2).to(torch.float32).contiguous()


def loader_statements(u8, pca=None, mean=MEAN, std=STD):
    """(image, normalised view), channels first, of uint8 views [...,H,W,3] in fp32: Flying3d.py:74-99's /255 and (x - mean) / std and,
    with pca (three floats), KITTI.py:171-191's lighting shift and clamp to 0..1 between them."""
    x = u8.movedim(-1, -3).float() / 255
    if pca is not None:
        x = x + pca.view(3, 1, 1)
        x = x.clamp(min=0, max=1)
    return x, (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
