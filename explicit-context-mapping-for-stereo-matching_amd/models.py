"""Drop-in mirror of the reference's `cmf.models` interface for the accelerated path.

Same class names, constructor signatures, attribute tree (=> identical `state_dict()` keys/shapes, so
reference checkpoints load), same `forward` signatures and return shapes as
`cmf/models/cmfsm.py` -- but every hot-path stage (cost volume, 3-D aggregation, soft-argmin, ECM
weights, ECM aggregation) runs on the gfx950 kernels in `ops.py`, and so do the 2-D encoder's convolutions and
GroupNorms; PyTorch-ROCm supplies the pooling / interpolation / concatenation glue around them.

Deliberate deviations (documented in DESIGN.md):
  * device-agnostic construction (no `.cuda()` inside modules, cf. cmfsm.py:98,117,427,671);
  * batch > 1 returns [B,1,H,W] (the reference broadcasts to [B,B,H,W], quirk Q1, cmfsm.py:714);
  * odd hr/lr scale raises ValueError instead of `exit()` (cmfsm.py:448-449);
  * the per-forward debug print + host sync (cmfsm.py:581-583) is dropped.
"""
from __future__ import annotations

import collections
import contextlib
import math
import numbers
import os as _os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import color as _color
from . import mesh as _mesh
from . import ops

NUM_GROUPS = 32  # cmfsm.py:31-33

# True: build the reference's explicit [B,2C,D',h,w] concat volume (ops.cost_volume) and run dres0's first Conv3d on it,
# exactly the reference's op sequence (cmfsm.py:667-684).  False (default): the same result from class-indexed 2-D
# convolutions of the feature maps without the 4-D tensor (ops.costvol_conv3d).  Env ECM_EXPLICIT_COST_VOLUME=1 or
# set `models.EXPLICIT_COST_VOLUME = True`.
EXPLICIT_COST_VOLUME = _os.environ.get("ECM_EXPLICIT_COST_VOLUME", "0") == "1"
# Nothing in this package falls back to a vendor library silently: a layer outside the native kernels raises unless
# ECM_ALLOW_FALLBACK=1, and every time a slower-than-designed path IS taken (that opt-in, or a dilated stage whose map is
# not divisible by its dilation and therefore runs on the direct dilated kernels instead of phase planes) an entry lands
# here and a warning is issued once per cause.
ALLOW_FALLBACK = _os.environ.get("ECM_ALLOW_FALLBACK", "0") == "1"
SLOW_PATH_EVENTS = []
_WARNED = set()


def _note_slow_path(kind, detail):
    SLOW_PATH_EVENTS.append((kind,) + tuple(detail))
    if kind not in _WARNED:
        _WARNED.add(kind)
        import warnings
        warnings.warn(f"ecm: {kind} {detail}: running on the slower native path (recorded in models.SLOW_PATH_EVENTS)")


# ------------------------------------------------------------------------------------------------
# leaf layers: nn.Conv3d / nn.ConvTranspose3d / nn.GroupNorm subclasses so parameter names, shapes and
# layouts are exactly the reference's, with forward() on the HIP kernels.
# ------------------------------------------------------------------------------------------------
class HipConv3d(nn.Conv3d):
    def forward(self, x, fork=False):
        """fork=True: returns (y, x') -- x' is x for the skip connection, its gradient folded into this layer's data-gradient
        kernel (ops._fork_out)."""
        return ops.conv3d_k3(x, self.weight, self.stride[0], fork)


class HipConvTranspose3d(nn.ConvTranspose3d):
    def forward(self, x):
        return ops.deconv3d_k3s2(x, self.weight)


class HipGroupNorm(nn.GroupNorm):
    """GroupNorm(32, C) on 5-D volumes; `fused()` adds the residual/ReLU the reference applies right after."""

    def forward(self, x):
        return ops.group_norm_act(x, self.weight, self.bias, None, False)

    def fused(self, x, skip=None, relu=False, head=0, out_dtype=None):
        if out_dtype is not None:                  # the boundary into the bf16 aggregation region (_costvol_dres0)
            return ops.group_norm_act(x, self.weight, self.bias, skip, relu, head, out_dtype)
        return ops.group_norm_act(x, self.weight, self.bias, skip, relu, head)


class HipReLU(nn.ReLU):
    """Placeholder keeping the reference's Sequential indices; fused into the preceding GroupNorm kernel."""


class EncConv2d(nn.Conv2d):
    """nn.Conv2d of the encoder (same parameters, hence the reference's state_dict keys).  Every layer shape of the
    registered architectures -- 3x3 with stride 1|2 and dilation 1|2|4, the 3-channel stem, the 64/128/320/384-channel
    stages, the 1x1 projections -- runs on the MFMA implicit-GEMM family (ops.conv2d: forward, data and weight gradient);
    a configuration outside it (none in the registered models) RAISES: the vendor-library path (nn.Conv2d's own forward on
    MIOpen) exists only behind ECM_ALLOW_FALLBACK=1, so a slow path can never be taken unseen."""

    def _native(self):
        kh, kw = self.kernel_size
        s, d = self.stride[0], self.dilation[0]
        return (self.groups == 1 and self.bias is None and self.stride[0] == self.stride[1]
                and self.dilation[0] == self.dilation[1] and self.padding == (d * (kh - 1) // 2, d * (kw - 1) // 2)
                and self.padding_mode == "zeros" and ops.conv2d_supported(self.in_channels, self.out_channels, kh, kw, s, d))

    def _native_bf16(self):
        kh, kw = self.kernel_size
        d = self.dilation[0]
        return (self.groups == 1 and self.bias is None and kh == kw and self.stride[0] == self.stride[1]
                and self.dilation[0] == self.dilation[1] and self.padding == (d * (kh - 1) // 2, d * (kw - 1) // 2)
                and self.padding_mode == "zeros" and ops.conv2d_bf16_supported(self.in_channels, self.out_channels, kh, self.stride[0], d))

    def forward(self, x, fork=False, out_dtype=None):
        """fork=True: returns (y, x') -- x' is x for the skip connection (ops._fork_out).
        A bf16 x (ops.encoder_dtype) runs the bf16 encoder kernel; out_dtype=torch.float32 writes its result in fp32."""
        if x.dtype == torch.bfloat16:
            if not self._native_bf16():
                raise RuntimeError(
                    f"EncConv2d({self.in_channels}->{self.out_channels}, k={self.kernel_size}, s={self.stride}, d={self.dilation}) "
                    "is outside the bf16 encoder kernel (ops.conv2d_bf16_supported); leave the encoder_dtype(torch.bfloat16) block")
            return ops.conv2d_bf16(x, self.weight, self.stride[0], self.dilation[0], fork,
                                   torch.bfloat16 if out_dtype is None else out_dtype)
        if x.dim() == 5:       # [B,C,d*d,H/d,W/d]: the phase planes of a dilation-d layer (feature_extraction._run_layer)
            return ops.conv2d_planes(x, self.weight, fork)
        if self._native():     # raises on CPU tensors, like every op
            return ops.conv2d(x, self.weight, self.stride[0], self.dilation[0], fork=fork)
        if not ALLOW_FALLBACK:
            raise RuntimeError(
                f"EncConv2d({self.in_channels}->{self.out_channels}, k={self.kernel_size}, s={self.stride}, d={self.dilation}, "
                f"groups={self.groups}, bias={self.bias is not None}) is outside the native 2-D family (ops.conv2d_supported); "
                "set ECM_ALLOW_FALLBACK=1 to run it on PyTorch-ROCm's own convolution instead")
        SLOW_PATH_EVENTS.append(("miopen_conv2d", self.in_channels, self.out_channels, self.kernel_size))
        y = super().forward(x)
        return (y, x) if fork else y


def convbn(in_planes, out_planes, kernel_size, stride, pad, dilation):
    """2-D conv + GroupNorm of the encoder (cmfsm.py:36-46): the convolution on the MFMA 2-D family (EncConv2d), the
    GroupNorm (and the ReLU / residual add that follows it) on the same fused HIP kernel as the 3-D stack."""
    return nn.Sequential(
        EncConv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride,
                  padding=dilation if dilation > 1 else pad, dilation=dilation, bias=False),
        HipGroupNorm(NUM_GROUPS, out_planes))


def _is_convbn(m):
    return isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[1], HipGroupNorm)


def _seq_fused(seq, x, start=0):
    """Run an encoder nn.Sequential (from module `start`), folding every `GroupNorm -> ReLU` pair into one fused launch."""
    mods = list(seq)
    i = start
    while i < len(mods):
        m = mods[i]
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        if _is_convbn(m):
            x = m[1].fused(m[0](x), None, relu)
            i += 2 if relu else 1
        elif isinstance(m, HipGroupNorm):
            x = m.fused(x, None, relu)
            i += 2 if relu else 1
        elif isinstance(m, nn.Sequential):
            x = _seq_fused(m, x)
            i += 1
        else:
            x = m(x)
            i += 1
    return x


def convbn_3d(in_planes, out_planes, kernel_size, stride, pad):
    """cmfsm.py:49-58: Sequential(Conv3d(bias=False), GroupNorm(32))."""
    if kernel_size != 3 or pad != 1:
        raise ValueError("the HIP path implements the reference's only configuration: kernel 3, pad 1")
    return nn.Sequential(
        HipConv3d(in_planes, out_planes, kernel_size=3, padding=1, stride=stride, bias=False),
        HipGroupNorm(NUM_GROUPS, out_planes))


def _costvol_dres0(dres0, lr_l, lr_r, ndisp):
    """Cost-volume build + dres0's first convbn_3d + ReLU (cmfsm.py:667-684) as one op: the reference-image half of the
    concat volume is constant along d, so its part of the convolution is a class-indexed set of 2-D convolutions of the
    feature map and only the shifted target-image half is materialised (ops.costvol_conv3d).  `ops.cost_volume` is the
    stand-alone builder of the full [B,2C,D,h,w] tensor (kept for the drop-in boundary and the microbench).
    Inside ops.aggregation_dtype(torch.bfloat16) the GroupNorm + ReLU writes bf16: the 3-D stack from here to the
    classifiers' 32 -> 1 layers then runs on the bf16 kernels (the ops dispatch on the volume's dtype)."""
    conv, gn = dres0[0][0], dres0[0][1]
    out_dtype = None
    if ops.aggregation_bf16():
        ops._AGG.guard("the bf16 aggregation stack")           # before the first 3-D launch
        out_dtype = torch.bfloat16
    if EXPLICIT_COST_VOLUME:
        return gn.fused(conv(ops.cost_volume(lr_l, lr_r, ndisp)), None, True, out_dtype=out_dtype)
    return gn.fused(ops.costvol_conv3d(lr_l, lr_r, conv.weight, ndisp), None, True, out_dtype=out_dtype)


def _cbn(seq, x, skip=None, relu=False, fork=False):
    """Run a convbn_3d Sequential with the trailing residual/ReLU fused into the GroupNorm kernel.
    fork=True: returns (out, x') where x' stands for x in the skip connection that also consumes it."""
    if fork:
        y, xs = seq[0](x, fork=True)
        return seq[1].fused(y, skip, relu), xs
    return seq[1].fused(seq[0](x), skip, relu)


# The tail of a classifier -- GroupNorm + ReLU + Conv3d(32 -> 1), cmfsm.py:621-634 -- as ONE op that never writes the
# normalised tensor (ops.classifier_tail).  ECM_C1_GN_FUSE=0 / models.C1_GN_FUSE = False: the three stages separately.
C1_GN_FUSE = _os.environ.get("ECM_C1_GN_FUSE", "1") != "0"


def _classifier(clf, x, fork=False):
    """clf = Sequential(convbn_3d(32, 32), ReLU, Conv3d(32, 1)).  -> raw logits [B,D,h,w] (and, with fork, x for the other
    consumer of the classifier's input, cf. _cbn)."""
    conv, gn, last = clf[0][0], clf[0][1], clf[2]
    if fork:
        y, xs = conv(x, fork=True)
    else:
        y, xs = conv(x), None
    if y.dtype == torch.bfloat16 or (C1_GN_FUSE and y.is_cuda and tuple(last.weight.shape) == (1, 32, 3, 3, 3)):   # bf16: the tail only
        out = ops.classifier_tail(y, gn.weight, gn.bias, last.weight).squeeze(1)
    else:
        out = last(gn.fused(y, None, True)).squeeze(1)
    return (out, xs) if fork else out


# ------------------------------------------------------------------------------------------------
# encoder (cmfsm.py:61-85, 126-236)
# ------------------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample, pad, dilation):
        super().__init__()
        self.conv1 = nn.Sequential(convbn(inplanes, planes, 3, stride, pad, dilation), nn.ReLU(inplace=True))
        self.conv2 = convbn(planes, planes, 3, 1, pad, dilation)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x, dual=False):
        """dual=True (bf16 encoder, the stage whose output leaves the encoder): returns (fp32 output, its bf16 copy) from one
        GroupNorm pass."""
        if self.downsample is None:
            # x feeds conv1 AND the residual add: conv1 hands x back so that its data gradient absorbs the skip gradient
            y, x = self.conv1[0][0](x, fork=True)
            out = self.conv1[0][1].fused(y, None, True)                    # GN + ReLU
        else:
            out = _seq_fused(self.conv1, x)                                # conv + GN + ReLU
            x = _seq_fused(self.downsample, x)
        if dual:
            gn = self.conv2[1]
            return ops.group_norm_act_bf16_f32(self.conv2[0](out), gn.weight, gn.bias, x, False, dual=True)
        return self.conv2[1].fused(self.conv2[0](out), x, False)            # conv + GN + residual add (cmfsm.py:76-85)


_INTERP_CACHE = {}


def _interp_matrix(n_in, n_out, device, dtype):
    """[n_out, n_in] weights of 1-D linear interpolation with align_corners=False (F.interpolate's source-index rule)."""
    key = (n_in, n_out, str(device), dtype)
    m = _INTERP_CACHE.get(key)
    if m is None:
        # fp32 source coordinates, exactly as ATen computes them (scale = in/out in float)
        dst = torch.arange(n_out, dtype=torch.float32)
        scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
        src = (scale * (dst + 0.5) - 0.5).clamp_(min=0.0)
        i0 = src.floor().long().clamp_(max=n_in - 1)
        i1 = (i0 + 1).clamp_(max=n_in - 1)
        l1 = (src - i0.float()).double()
        m = torch.zeros(n_out, n_in, dtype=torch.float64)
        m.scatter_add_(1, i0.unsqueeze(1), (1.0 - l1).unsqueeze(1))
        m.scatter_add_(1, i1.unsqueeze(1), l1.unsqueeze(1))
        m = m.to(device=device, dtype=dtype)
        _INTERP_CACHE[key] = m
    return m


def bilinear_upsample(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) of the tiny SPP branch maps (cmfsm.py:208-229) as two
    small matmuls with the separable interpolation matrices: same values, but the backward is a matmul instead of
    ATen's atomic scatter (2 ms per call at 144x240 from a 2x3 map)."""
    H, W = size
    if x.dtype == torch.bfloat16:        # bf16 encoder: interpolate in fp32 (weights not rounded), round the result once
        return bilinear_upsample(x.float(), size).to(torch.bfloat16)
    uy = _interp_matrix(x.shape[-2], H, x.device, x.dtype)
    ux = _interp_matrix(x.shape[-1], W, x.device, x.dtype)
    return torch.matmul(uy, torch.matmul(x, ux.t()))


# Encoder variants of the registered architectures (all plain PyTorch):
#   first_tail  "conv": firstconv ends with a bare Conv2d and secondconv starts with GroupNorm+ReLU (cmfsm.py:130-145,
#               cm_sub_4.py, bilinear_cmf.py);  "convbn": firstconv ends with convbn+ReLU (cmfsm_sub_8.py:131-145 ...)
#   layers      (stride, dilation) of layer1..4;  pools: AvgPool sizes of branch1..4;  cat_raw: which map joins the
#   pyramid as "output_raw" (layer2 output, or layer3 output for the /16 nets whose last conv is `lastconv_16`).
_ENCODERS = {
    "cmfsm": dict(first_tail="conv", layers=((1, 1), (2, 1), (1, 1), (1, 2)), pools=(64, 32, 16, 8), raw="layer2"),
    "sub4": dict(first_tail="conv", layers=((1, 1), (2, 1), (1, 2), (1, 4)), pools=(64, 32, 16, 8), raw="layer2"),
    "sub8": dict(first_tail="convbn", layers=((2, 1), (2, 1), (1, 2), (1, 4)), pools=(4, 32, 16, 8), raw="layer2"),
    "sub16": dict(first_tail="convbn", layers=((2, 1), (2, 1), (2, 1), (1, 4)), pools=(4, 2, 16, 8), raw="layer3"),
    # cmf.py:126-225: stride-2 stem of three convbn+ReLU, no secondconv; layer1's output (1/2 resolution) is the decoder's `half`
    "cmf": dict(first_tail="none", stem_stride=2, layers=((1, 1), (2, 1), (1, 1), (1, 2)), pools=(64, 32, 16, 8), raw="layer2"),
}


def _pyramid_pools(x, pools):
    """The SPP branches' AvgPool2d(k, stride k) of the SAME map (cmfsm.py:152-170) computed hierarchically: the smallest
    window reads the map once, every larger window that is a multiple of a smaller one pools that result (same windows:
    floor(floor(n/a)/r) == floor(n/(a*r)); only the summation order inside a window changes).  The reference reads the
    128-channel map once per branch.  `pools`: the branches' nn.AvgPool2d modules; returns their outputs in that order."""
    ks = [int(p.kernel_size[0] if isinstance(p.kernel_size, tuple) else p.kernel_size) for p in pools]
    done = {}
    for k in sorted(set(ks)):
        base = max((j for j in done if k % j == 0), default=None)
        done[k] = F.avg_pool2d(x, k, k) if base is None else F.avg_pool2d(done[base], k // base, k // base)
    return [done[k] for k in ks]


class feature_extraction(nn.Module):
    """Returns (low-res 32-ch feature, layer1 output, full-res 32-ch firstconv output)  (cmfsm.py:126-236 and the
    per-architecture copies: cmfsm_sub_8.py:126-236, cmfsm_sub_16.py:127-239, cm_sub_4.py:126-236).  Variant "cmf"
    (cmf.py:126-225, no full-resolution map): the third result is layer1's output (1/2 resolution) again, or with `head`
    its first `head` samples."""

    def __init__(self, variant="cmfsm"):
        super().__init__()
        cfg = _ENCODERS[variant]
        self.variant = variant
        self.inplanes = 32
        head = [convbn(3, 32, 3, cfg.get("stem_stride", 1), 1, 1), nn.ReLU(inplace=True),
                convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True),
                convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True)]
        if cfg["first_tail"] == "none":
            self.firstconv = nn.Sequential(*head)
        elif cfg["first_tail"] == "conv":
            self.firstconv = nn.Sequential(*head, EncConv2d(32, 32, kernel_size=3, padding=1, stride=1, bias=False))
            self.secondconv = nn.Sequential(
                HipGroupNorm(NUM_GROUPS, 32), nn.ReLU(inplace=True),
                convbn(32, 32, 3, 2, 1, 1), nn.ReLU(inplace=True),
                convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True))
        else:
            self.firstconv = nn.Sequential(*head, convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True))
            self.secondconv = nn.Sequential(
                convbn(32, 32, 3, 2, 1, 1), nn.ReLU(inplace=True),
                convbn(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True))
        (s1, d1), (s2, d2), (s3, d3), (s4, d4) = cfg["layers"]
        self.layer1 = self._make_layer(BasicBlock, 32, 3, s1, 1, d1)
        self.layer2 = self._make_layer(BasicBlock, 64, 16, s2, 1, d2)
        self.layer3 = self._make_layer(BasicBlock, 128, 3, s3, 1, d3)
        self.layer4 = self._make_layer(BasicBlock, 128, 3, s4, 1, d4)
        for i, pool in enumerate(cfg["pools"], 1):
            setattr(self, f"branch{i}", nn.Sequential(
                nn.AvgPool2d((pool, pool), stride=(pool, pool)), convbn(128, 32, 1, 1, 0, 1), nn.ReLU(inplace=True)))
        last = nn.Sequential(
            convbn(320 if cfg["raw"] == "layer2" else 384, 128, 3, 1, 1, 1), nn.ReLU(inplace=True),
            EncConv2d(128, 32, kernel_size=1, padding=0, stride=1, bias=False))
        setattr(self, "lastconv" if cfg["raw"] == "layer2" else "lastconv_16", last)
        self._raw_is_layer3 = cfg["raw"] == "layer3"
        self._first_tail = cfg["first_tail"]

    def _make_layer(self, block, planes, blocks, stride, pad, dilation):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                EncConv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                HipGroupNorm(NUM_GROUPS, planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, pad, dilation)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes, 1, None, pad, dilation) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    @staticmethod
    def _run_layer(layer, x):
        """One residual stage.  If every convolution in it is a 3x3 / stride 1 layer of the same dilation d > 1 (cmfsm's
        layer4, cmfsm.py:150), run it on d*d phase planes, where the convolutions are ordinary 3x3 ones (ops.phase_split)."""
        if x.dtype == torch.bfloat16:     # bf16 encoder: the kernel runs the dilation natively, no phase planes
            return layer(x)
        convs = [m for m in layer.modules() if isinstance(m, nn.Conv2d)]
        d = convs[0].dilation[0]
        ok = (ops.WINOGRAD and d > 1 and x.shape[-2] % d == 0 and x.shape[-1] % d == 0 and x.shape[-1] // d >= 2
              and all(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.dilation == (d, d) and m.padding == (d, d) for m in convs))
        if not ok:
            if d > 1 and ops.WINOGRAD:
                # still this library's kernels (the direct dilated 3x3 family), but not the designed fast path: made visible.
                # Only a map whose height / width is not a multiple of the dilation gets here (e.g. the /16 nets' dilation-4
                # stage on a 384x1248 KITTI frame: 24 x 78); no registered architecture does at the SceneFlow size.
                _note_slow_path("dilated_stage_unphased", (d, tuple(x.shape)))
            return layer(x)
        return ops.phase_merge(layer(ops.phase_split(x, d)), d)

    def _tail(self, x, out_dtype=None):
        """layer2 -> layer3/4 -> pooled pyramid -> last conv: layer1's output -> the low-resolution 32-channel feature.
        `out_dtype` (bf16 encoder): the final 1x1 writes its result in that dtype instead of x's."""
        output_raw = self.layer2(x)
        if self._raw_is_layer3:                       # cmfsm_sub_16.py:205-207
            output_raw = self._run_layer(self.layer3, output_raw)
            output_skip = self._run_layer(self.layer4, output_raw)
        else:
            output_skip = self._run_layer(self.layer4, self._run_layer(self.layer3, output_raw))
        size = output_skip.shape[-2:]
        pooled = _pyramid_pools(output_skip, [getattr(self, f"branch{i}")[0] for i in (1, 2, 3, 4)])
        pyramid = [bilinear_upsample(_seq_fused(getattr(self, f"branch{i}"), pooled[i - 1], start=1), size) for i in (4, 3, 2, 1)]
        last = list(self.lastconv_16 if self._raw_is_layer3 else self.lastconv)
        h = _seq_fused(last[:-1], torch.cat([output_raw, output_skip] + pyramid, 1))
        return last[-1](h) if out_dtype is None else last[-1](h, out_dtype=out_dtype)

    def forward(self, x, head=None):
        """`head` (extension): the caller only needs the first `head` samples of the full-resolution map (third result); their
        gradient is then folded into the map's gradient in place (ops.fork_head) instead of through a zero-padded copy.
        Inside ops.encoder_dtype(torch.bfloat16): _forward_bf16."""
        if ops.encoder_bf16():
            return self._forward_bf16(x, head)
        output_all = _seq_fused(self.firstconv, x)
        output_head = None
        if not hasattr(self, "secondconv"):           # cmf.py:197-198: firstconv -> layer1 directly
            output_rt = self.layer1(output_all)
            output_all = output_rt
            if head is not None:
                output_rt, output_head = ops.fork_head(output_rt, head)
        elif head is not None and isinstance(self.secondconv[0], HipGroupNorm):
            # the map's whole-batch consumer is secondconv's GroupNorm + ReLU: that node hands the head slice out and folds
            # its gradient into its own data gradient (ops.GroupNormAct `head`)
            y, output_head = self.secondconv[0].fused(output_all, None, True, head=head)
            output_rt = self.layer1(_seq_fused(self.secondconv, y, start=2))
        else:
            if head is not None:
                output_all, output_head = ops.fork_head(output_all, head)
            output_rt = self.layer1(_seq_fused(self.secondconv, output_all))
        feature = self._tail(output_rt)
        return feature, output_rt, (output_all if output_head is None else output_head)

    @staticmethod
    def _layer_dual(layer, x):
        """A residual stage whose output is an encoder result: -> (fp32 output, bf16 copy for the next stage)."""
        blocks = list(layer)
        for blk in blocks[:-1]:
            x = blk(x)
        return blocks[-1](x, dual=True)

    def _forward_bf16(self, x, head=None):
        """The encoder on bf16 maps (ops.encoder_dtype): the 3 -> 32 stem convolution reads the fp32 image and stays fp32, its
        GroupNorm + ReLU writes bf16; every later layer runs on the bf16 kernels (a layer outside them raises).  The three
        results are written in fp32 by the kernel that produces them: the full-resolution map by firstconv's bare last
        convolution ("conv" variants) or by a GroupNorm that also writes the bf16 copy the next layer reads ("convbn"); layer1's
        output the same way; the low-resolution feature by lastconv's 1x1.  `head`: a slice of the fp32 map (no autograd)."""
        ops._ENC.no_grad("feature_extraction")                  # before the first launch
        bf = torch.bfloat16
        fc = list(self.firstconv)
        conv0, gn0 = fc[0][0], fc[0][1]
        h = gn0.fused(conv0(x), None, True, out_dtype=bf)
        if self._first_tail == "conv":
            h = _seq_fused(fc[2:-1], h)
            output_all = fc[-1](h, out_dtype=torch.float32)
            h = _seq_fused(self.secondconv, self.secondconv[0].fused(output_all, None, True, out_dtype=bf), start=2)
            output_rt, h = self._layer_dual(self.layer1, h)
        elif self._first_tail == "convbn":
            h = _seq_fused(fc[2:-2], h)
            conv, gn = fc[-2][0], fc[-2][1]
            output_all, h = ops.group_norm_act_bf16_f32(conv(h), gn.weight, gn.bias, None, True, dual=True)
            output_rt, h = self._layer_dual(self.layer1, _seq_fused(self.secondconv, h))
        else:                                                   # "none" (cmf): layer1's output is the map
            output_rt, h = self._layer_dual(self.layer1, _seq_fused(fc[2:], h))
            output_all = output_rt
        feature = self._tail(h, out_dtype=torch.float32)
        return feature, output_rt, (output_all if head is None else output_all[:head])


# ------------------------------------------------------------------------------------------------
# hot-path modules
# ------------------------------------------------------------------------------------------------
class matchshifted(nn.Module):
    """One disparity slice of the cost volume, [B,2C,1,H,W] (cmfsm.py:88-108; unused by the reference's forward)."""

    def forward(self, left, right, shift):
        return ops.cost_volume(left, right, shift + 1)[:, :, shift:shift + 1]


class disparityregression(nn.Module):
    """sum_d x[:,d]*d (cmfsm.py:111-123)."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = maxdisp

    def forward(self, x):
        return ops.disparity_regression(x)


class hourglass(nn.Module):
    """cmfsm.py:240-303."""

    def __init__(self, inplanes):
        super().__init__()
        c2 = inplanes * 2
        self.conv1 = nn.Sequential(convbn_3d(inplanes, c2, kernel_size=3, stride=2, pad=1), HipReLU(inplace=True))
        self.conv2 = convbn_3d(c2, c2, kernel_size=3, stride=1, pad=1)
        self.conv3 = nn.Sequential(convbn_3d(c2, c2, kernel_size=3, stride=2, pad=1), HipReLU(inplace=True))
        self.conv4 = nn.Sequential(convbn_3d(c2, c2, kernel_size=3, stride=1, pad=1), HipReLU(inplace=True))
        self.conv5 = nn.Sequential(
            HipConvTranspose3d(c2, c2, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False),
            HipGroupNorm(NUM_GROUPS, c2))
        self.conv6 = nn.Sequential(
            HipConvTranspose3d(c2, inplanes, kernel_size=3, padding=1, output_padding=(1, 1, 1), stride=2, bias=False),
            HipGroupNorm(NUM_GROUPS, inplanes))

    def forward(self, x, presqu, postsqu, residual=None, pre_uses=1):
        """`residual` (extension): added to `out` inside the last GroupNorm kernel (cmfsm.py:687,690,693).
        `pre_uses` (extension): how many times the CALLER will consume the returned `pre`; with more than one consumer in all
        (conv3, the skip of conv5 when `presqu` is None, the caller's) their gradients are summed by one kernel (ops.fork)
        instead of one autograd add each, and `pre` is returned as a tuple of `pre_uses` aliases."""
        out = _cbn(self.conv1[0], x, relu=True)                                   # :285
        pre = _cbn(self.conv2, out, skip=postsqu, relu=True)                      # :286-290
        inner = 2 if presqu is None else 1
        views = ops.fork(pre, inner + pre_uses) if pre_uses > 1 else (pre,) * (inner + pre_uses)
        out = _cbn(self.conv3[0], views[0], relu=True)                            # :292
        out = _cbn(self.conv4[0], out, relu=True)                                 # :293
        post = _cbn(self.conv5, out, skip=presqu if presqu is not None else views[1], relu=True)   # :295-299
        out = _cbn(self.conv6, post, skip=residual, relu=False)                   # :301
        return out, (pre if pre_uses <= 1 else tuple(views[inner:])), post


class similarity_measure1(nn.Module):
    """Per-pixel MLP as 1x1 convs 66->32->16->8->1, LeakyReLU between, no bias (cmfsm.py:304-358).
    Parameter holder for the fused ECM-weights kernel; calling it directly runs the plain 1x1 convs."""

    def __init__(self):
        super().__init__()
        self.inplanes = 32
        self.conv0 = nn.Conv2d(66, 32, kernel_size=1, bias=False)
        self.relu0 = nn.LeakyReLU(inplace=True)
        self.conv1 = nn.Conv2d(32, 16, kernel_size=1, bias=False)
        self.relu1 = nn.LeakyReLU(inplace=True)
        self.conv2 = nn.Conv2d(16, 8, kernel_size=1, bias=False)
        self.relu2 = nn.LeakyReLU(inplace=True)
        self.conv3 = nn.Conv2d(8, 1, kernel_size=1, bias=False)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = self.relu0(self.conv0(x))
        x = self.relu1(self.conv1(x))
        x = self.relu2(self.conv2(x))
        return self.conv3(x)


class eight_related_context_mapping(nn.Module):
    """cmfsm.py:431-593 -> nine softmax planes [B,1,H,W] (centre,l,r,t,b,lt,rt,lb,rb)."""

    def __init__(self):
        super().__init__()
        self.similarity1 = similarity_measure1()
        self.sigmoid = nn.Sigmoid()

    def weights(self, lr_feature, hr_feature):
        m = self.similarity1
        return ops.ecm_weights9(lr_feature, hr_feature, m.conv0.weight, m.conv1.weight, m.conv2.weight, m.conv3.weight)

    def forward(self, lr_feature, hr_feature, lr_feature_r=None, hr_feature_r=None):
        w9 = self.weights(lr_feature, hr_feature)          # right-image inputs are ignored (cmfsm.py:474-480)
        return tuple(w9[:, n:n + 1] for n in range(9))


class similarity_measure2(nn.Module):
    """3->3->2->1 1x1-conv MLP on the offset table (cm_sub_4.py: instantiated, never used in forward)."""

    def __init__(self):
        super().__init__()
        self.inplanes = 32
        self.conv0 = nn.Conv2d(3, 3, kernel_size=1, bias=False)
        self.relu0 = nn.LeakyReLU(inplace=True)
        self.conv1 = nn.Conv2d(3, 2, kernel_size=1, bias=False)
        self.relu1 = nn.LeakyReLU(inplace=True)
        self.conv2 = nn.Conv2d(2, 1, kernel_size=1, bias=False)
        self.relu2 = nn.LeakyReLU(inplace=True)

    def forward(self, x):
        return self.relu2(self.conv2(self.relu1(self.conv1(self.relu0(self.conv0(x))))))


class six_related_context_mapping(nn.Module):
    """cmfsm_sub_8.py:440-572 (same text in cmfsm_sub_16.py and cm_sub_4/8/16.py):
    forward(lr, hr, lr_r, hr_r) -> ((mapping, mapping_r, mapping_l, mapping_t, mapping_b),
                                    (mapping_target, mapping_target_r, mapping_target_l)), each [B,1,H,W]."""

    def __init__(self, with_similarity2=False):
        super().__init__()
        self.similarity1 = similarity_measure1()
        self.similarity1.relu3 = nn.LeakyReLU(inplace=True)          # cmfsm_sub_8.py:318 (no parameters)
        if with_similarity2:
            self.similarity2 = similarity_measure2()                 # cm_sub_4.py only; unused in forward
        self.fuse = nn.Sequential(nn.Conv2d(2, 1, kernel_size=1, bias=False), nn.LeakyReLU(inplace=True))   # unused

    def planes(self, lr_feature, hr_feature, lr_feature_r, hr_feature_r):
        m = self.similarity1
        ws = (m.conv0.weight, m.conv1.weight, m.conv2.weight, m.conv3.weight)
        return (ops.context_weights(lr_feature, hr_feature, *ws, 1), ops.context_weights(lr_feature_r, hr_feature_r, *ws, 2))

    def forward(self, lr_feature, hr_feature, lr_feature_r, hr_feature_r):
        m5, mt3 = self.planes(lr_feature, hr_feature, lr_feature_r, hr_feature_r)
        return tuple(m5[:, n:n + 1] for n in range(5)), tuple(mt3[:, n:n + 1] for n in range(3))


# What _ECMNet.predict returns: per requested head, the disparity and the standard deviation (pixels), peak probability and
# entropy (nats) of the distribution whose mean it is; each field a tuple of [B,1,H,W] tensors.
Prediction = collections.namedtuple("Prediction", "disparity std peak entropy")
# ... and with predict(mode_radius=r): what to use where those say the mean cannot be trusted: the mean of
# that distribution inside the window of r pixels about its highest level (`mode`, pixels), the window's share of the
# distribution (`mass`) and the highest level itself (`index`, pixels).  The first four fields are Prediction's, bit for bit.
ModalPrediction = collections.namedtuple("ModalPrediction", "disparity std peak entropy mode mass index")

# The fields of a prediction that _ECMNet.sparsification ranks the errors by: for the first two a higher
# value means less trusted, the last two are negated; "mass" exists only with a mode_radius.
SPARSIFICATION_MEASURES = ("std", "entropy", "peak", "mass")

# What _ECMNet.cross_check returns, each field [B,1,H,W]: one head's disparity of the left view and of
# the right view (in right-image coordinates), the left-right error (pixels), the failure class (0 consistent, 1 occluded,
# 2 mismatch, 3 out of view; a float plane) and the left disparity with the failures filled from the background.
CrossCheck = collections.namedtuple("CrossCheck", "disparity disparity_right error kind filled")

# Where the disparity_right of refine, despeckle and smooth comes from: "cross", a second forward on the
# flipped and swapped pair (cross_check: the default), or "splat", the left disparity forward-warped into the right view
# (self_check: one forward).  Chosen by the occlusion_check block below; cross_check and self_check themselves do not look at it.
CHECKS = ("cross", "splat")
_CHECK = "cross"


@contextlib.contextmanager
def occlusion_check(check):
    """"cross" (the default; a no-op) or "splat": inside the block refine, despeckle and smooth of every model start from
    self_check -- one forward and ops.disparity_splat -- instead of cross_check's two forwards, with self_check's limits: no
    mismatch class, only the occlusions the left map's own geometry implies, up to one extra column at an occlusion edge, and an
    effect on EPE or D1 that nobody has measured.  Anything else raises ValueError on entry, before any device work.  Nests and
    restores the previous setting on exit."""
    global _CHECK
    if check not in CHECKS:
        raise ValueError(f"occlusion_check: check {check!r}: one of {CHECKS}")
    prev, _CHECK = _CHECK, check
    try:
        yield
    finally:
        _CHECK = prev


# What _ECMNet.refine returns: CrossCheck's five fields, bit for bit, then the masked median of `filled`
# and the joint bilateral filter of that median guided by the left image, each [B,1,H,W].
Refined = collections.namedtuple("Refined", "disparity disparity_right error kind filled median refined")

# What _ECMNet.despeckle returns: Refined's seven fields in the same order -- the first
# five cross_check's bit for bit, the two filters reading `despeckled` -- then the filled map without the small segments and the
# segment size of every pixel (int32; 0 where the pixel is not consistent), each [B,1,H,W].
Despeckled = collections.namedtuple("Despeckled", Refined._fields + ("despeckled", "segment"))

# What _ECMNet.smooth returns: CrossCheck's five fields bit for bit, then the confidence plane the smoother
# was given (1.0 where the pixel is consistent and, with the speckle filter on, in a segment larger than speckle_size; else 0) and
# the WLS-smoothed disparity, each [B,1,H,W].
Smoothed = collections.namedtuple("Smoothed", CrossCheck._fields + ("confidence", "smoothed"))

# What _ECMNet.point_cloud returns: the packed cloud [N, 3 + C] and its offsets [B + 1] (int64), the dense
# point map [B,3,H,W] and its mask [B,H,W] (bool), and `stage`: the result of the entry point named by `source`, bit for bit.
PointCloud = collections.namedtuple("PointCloud", "points offsets xyz mask stage")

# source -> the field of that entry point's result that is reprojected (None: head 2 of forward's tuple, every pixel valid)
POINT_CLOUD_SOURCES = {"forward": None, "self_check": "filled", "cross_check": "filled", "refine": "refined", "despeckle": "refined",
                       "smooth": "smoothed"}

_NO_DISTRIBUTION = {
    "five": "the full-resolution disparity of this head is a sum of low-resolution disparities weighted by softmax * logit planes: "
            "signed weights that do not sum to one, so it is not the mean of any distribution over disparities",
    "srr": "a refinement decoder follows the soft-argmin heads: the full-resolution disparity is the decoder's output, and no "
           "distribution over disparities exists there",
}


_MODE_OP = {"eight": ops.ecm_aggregate9_mode, "volume": ops.volume_mapping_mode, "trilinear": ops.trilinear_softargmin_mode}


class _ECMNet(nn.Module):
    """Shared skeleton of the registered architectures: encoder -> cost volume -> dres0/1 -> 1 or 3 hourglasses ->
    classifiers (`_aggregate`) -> head (`hot_path`).  Subclasses set ENCODER, HOURGLASSES and HEAD exactly as their reference
    file does.  PRE1_FORK: the first hourglass's `pre` has four consumers in a three-hourglass net (two inside that
    hourglass, the skips of the other two); True sums their gradients with one ops.fork kernel, False leaves the sum to
    autograd.  The two orders of summation differ in the last bit, so the attribute is part of each net's definition."""
    ENCODER, HOURGLASSES, HEAD, SIM2, PRE1_FORK = "cmfsm", 3, "eight", False, False
    LEVEL_SPACING = 1      # full-resolution pixels between two levels of the head's distribution (a mode radius is a multiple)

    def __init__(self, maxdisp=192):
        super().__init__()
        self.maxdisp = maxdisp
        self.feature_extraction = feature_extraction(self.ENCODER)
        self.dres0 = nn.Sequential(convbn_3d(64, 32, 3, 1, 1), HipReLU(inplace=True),
                                   convbn_3d(32, 32, 3, 1, 1), HipReLU(inplace=True))
        self.dres1 = nn.Sequential(convbn_3d(32, 32, 3, 1, 1), HipReLU(inplace=True),
                                   convbn_3d(32, 32, 3, 1, 1))
        for i in range(self.HOURGLASSES):
            setattr(self, f"dres{i + 2}", hourglass(32))
        for i in range(self.HOURGLASSES):
            setattr(self, f"classif{i + 1}", nn.Sequential(
                convbn_3d(32, 32, 3, 1, 1), HipReLU(inplace=True),
                HipConv3d(32, 1, kernel_size=3, padding=1, stride=1, bias=False)))
        if self.HEAD == "eight":
            self.mapping_matrix = eight_related_context_mapping()
        elif self.HEAD in ("five", "volume"):
            self.mapping_matrix = six_related_context_mapping(self.SIM2)
        for m in self.modules():                                      # PSMNet init rule, e.g. cmfsm.py:638-645
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
            elif isinstance(m, nn.Conv3d):
                k = m.kernel_size
                m.weight.data.normal_(0, math.sqrt(2.0 / (k[0] * k[1] * k[2] * m.out_channels)))

    def _aggregate(self, lr_l, lr_r, ndisp):
        """The 3-D trunk (cmfsm.py:667-693 and every classifier's layers): cost volume -> dres0 -> dres1 -> the hourglasses
        chained through the first one's `pre` and the previous one's `post` -> the classifiers.
        Returns the list of raw classifier outputs [B,ndisp,h,w], one per hourglass."""
        n = self.HOURGLASSES
        cost0 = _costvol_dres0(self.dres0, lr_l, lr_r, ndisp)                          # :667-684
        cost0 = _cbn(self.dres0[2], cost0, relu=True)
        y, cost0 = _cbn(self.dres1[0], cost0, relu=True, fork=True)                    # :685
        cost0 = _cbn(self.dres1[2], y, skip=cost0)
        # cost0's consumers (first hourglass + one residual add per hourglass): one n-ary gradient sum instead of n adds
        c_forks = ops.fork(cost0, n + 1)
        pre_uses = max(n - 1, 1) if self.PRE1_FORK else 1
        heads, x, post = [], c_forks[0], None
        for i in range(n):
            if i == 0:
                out, pre, post = self.dres2(x, None, None, residual=c_forks[1], pre_uses=pre_uses)    # :686-687
                pre1 = pre if pre_uses > 1 else (pre,) * (n - 1)          # one alias of `pre` per later hourglass
            else:
                out, _, post = getattr(self, f"dres{i + 2}")(x, pre1[i - 1], post, residual=c_forks[i + 1])   # :689-693
            # `out` feeds the next hourglass AND its classifier: the classifier's first convolution hands it back (fork), so
            # that its data gradient absorbs the gradient arriving through the hourglass
            clf = getattr(self, f"classif{i + 1}")
            if i + 1 < n:
                c_i, x = _classifier(clf, out, fork=True)
            else:
                c_i = _classifier(clf, out)
            heads.append(c_i)
        return heads

    def hot_path(self, lr_l, hr_l, lr_r, hr_r, out_hw=None):
        scale = hr_l.shape[-1] // lr_l.shape[-1]
        planes = None
        if self.HEAD in ("five", "volume"):
            planes = self.mapping_matrix.planes(lr_l, hr_l, lr_r, hr_r)
        c = torch.stack(self._aggregate(lr_l, lr_r, self.maxdisp // scale), 0)   # raw classifier outputs [NH,B,Dl,h,w]
        if self.HEAD == "five":                                          # cmfsm_sub_8.py:757-803 (heads NOT accumulated)
            disp = torch.cat([ops.softargmin_heads(c[k:k + 1]) for k in range(c.shape[0])], 0)
            m5 = planes[0]
            w9 = torch.cat([m5[:, 0:1], m5[:, 2:3], m5[:, 1:2], m5[:, 3:5], torch.zeros_like(m5[:, :4])], 1)
            preds = ops.ecm_aggregate9(disp, w9, scale)                  # planes reordered c,l,r,t,b + 4 zero diagonals
            return tuple(preds[k].unsqueeze(1) for k in range(3))
        if self.HEAD == "volume":                                        # cmfsm_sub_16.py:767-848 / cm_sub_8.py:765-800
            preds = ops.volume_mapping(c, planes[0], planes[1], scale)
        else:                                                            # bilinear_cmf.py:447-471
            H, W = out_hw if out_hw is not None else hr_l.shape[-2:]
            preds = ops.trilinear_softargmin(c, self.maxdisp, H, W)
        preds = [preds[k] for k in range(preds.shape[0])]
        while len(preds) < 3:                                            # cm_sub_*: `return pred1, pred1, pred1`
            preds.append(preds[0])
        return tuple(preds)

    def forward(self, left, right):
        B = left.shape[0]
        if torch.is_grad_enabled():
            ops.pace_side_streams()
        lr, _, hr = self.feature_extraction(torch.cat([left, right], 0))      # one encoder pass for both images
        return self.hot_path(lr[:B], hr[:B], lr[B:], hr[B:], out_hw=left.shape[-2:])

    def head_stats(self, left, right):
        """One forward up to the head, then the head with its statistics: (disp, std, peak, entropy), each [NH,B,H,W] for the
        NH classifiers of the net, and the head's operands (what ops.*_stats was called with), for predict()."""
        B = left.shape[0]
        lr, _, hr = self.feature_extraction(torch.cat([left, right], 0))
        lr_l, hr_l, lr_r, hr_r = lr[:B], hr[:B], lr[B:], hr[B:]
        scale = hr_l.shape[-1] // lr_l.shape[-1]
        planes = self.mapping_matrix.planes(lr_l, hr_l, lr_r, hr_r) if self.HEAD == "volume" else None
        c = torch.stack(self._aggregate(lr_l, lr_r, self.maxdisp // scale), 0)
        if self.HEAD == "volume":
            args = (c, planes[0], planes[1], scale)
            return ops.volume_mapping_stats(*args), args
        args = (c, self.maxdisp, *left.shape[-2:])
        return ops.trilinear_softargmin_stats(*args), args

    def predict(self, left, right, heads=None, mode_radius=None):
        """One inference forward that also says how sure each disparity is: a Prediction whose .disparity, .std, .peak and
        .entropy are tuples of [B,1,H,W], one entry per head in `heads` (default: all three; the one-hourglass nets repeat
        their single head as forward does).  .disparity is bit-identical to forward's under torch.no_grad().  All classifiers
        run whatever `heads` says -- head k's logits are c_0 + ... + c_k -- and the head kernel is launched for all of them:
        a launch for fewer heads is another template instantiation, which need not round like forward's.  Forward only.
        With mode_radius = r (an integer >= 0 in full-resolution pixels, a multiple of LEVEL_SPACING) the result is a
        ModalPrediction: the same four fields, bit for bit, plus .mode, .mass and .index of the window of r pixels about the
        highest level of each head's distribution, from one more head kernel on the same logits."""
        if self.HEAD in _NO_DISTRIBUTION:                                # before any device work
            raise NotImplementedError(f"{type(self).__name__}.predict: {_NO_DISTRIBUTION[self.HEAD]}")
        heads = (0, 1, 2) if heads is None else tuple(int(k) for k in heads)
        if not heads or any(k < 0 or k > 2 for k in heads):
            raise ValueError(f"predict: heads {heads}: a non-empty selection of 0, 1, 2")
        if mode_radius is not None:                                      # also before any device work
            mode_radius = ops.check_mode_radius(mode_radius, self.LEVEL_SPACING)
        with torch.no_grad():
            fields, args = self.head_stats(left, right)
            kind = Prediction
            if mode_radius is not None:
                kind, fields = ModalPrediction, tuple(fields) + tuple(_MODE_OP[self.HEAD](*args, mode_radius))
        last = fields[0].shape[0] - 1
        return kind(*(tuple(f[min(k, last)].unsqueeze(1) for k in heads) for f in fields))

    def sparsification(self, left, right, gt, head=2, measures=("std", "entropy", "peak"), mode_radius=None, steps=20, maxdisp=192):
        """Do the confidence outputs rank this net's errors?  One predict forward (with mode_radius, so that "mass" can be among
        the measures when it is given) and ops.eval_sparsification of head `head`'s disparity against gt [B,H,W] with the named
        fields as the measures -- "peak" and "mass" negated, since for those a higher value means MORE trusted.  Returns
        (prediction, Sparsification): the prediction is predict(left, right, (head,), mode_radius), bit for bit; the curves and
        areas are in the order of `measures`.  The curves say how well each measure orders the errors of THIS input; they say
        nothing about how large the errors are, and with untrained weights nothing about which measure is best."""
        if self.HEAD in _NO_DISTRIBUTION:                                # predict's refusal, before any device work
            raise NotImplementedError(f"{type(self).__name__}.predict: {_NO_DISTRIBUTION[self.HEAD]}")
        if isinstance(head, bool) or not isinstance(head, numbers.Integral) or not 0 <= head <= 2:
            raise ValueError(f"sparsification: head {head!r}: one of 0, 1, 2")
        measures = (measures,) if isinstance(measures, str) else tuple(measures)
        known = SPARSIFICATION_MEASURES if mode_radius is not None else SPARSIFICATION_MEASURES[:3]
        for name in measures:
            if name not in known:
                raise ValueError(f"sparsification: measure {name!r}: one of {known}" +
                                 ("" if mode_radius is not None else ' ("mass" needs a mode_radius)'))
        steps, maxdisp = ops.check_sparsification_parameters(len(measures), steps, maxdisp, "sparsification")
        prediction = self.predict(left, right, (int(head),), mode_radius)
        planes = [getattr(prediction, name)[0] for name in measures]
        planes = [-m if name in ("peak", "mass") else m for name, m in zip(measures, planes)]
        return prediction, ops.eval_sparsification(prediction.disparity[0], gt, planes, maxdisp, steps)

    def cross_check(self, left, right, threshold=1.0, rel=0.0, head=2):
        """The left-right consistency check of one head: two plain inference forwards -- (left, right), and the two images
        flipped along W and swapped, which gives the right view's disparity mirrored -- and one ops.lr_check kernel on the two
        planes.  Returns a CrossCheck; .disparity is bit-identical to forward's under torch.no_grad(), .disparity_right to the
        flipped forward's, flipped back once for the caller (the kernel reads the mirrored plane as it is).  Needs `forward`
        only, so every registered architecture has it.  threshold (pixels) and rel (a share of the disparity) as in
        ops.lr_check; head in 0..2."""
        return self._cross_check(left, right, threshold, rel, head, False, "cross")[0]

    def self_check(self, left, right, threshold=1.0, rel=0.0, head=2):
        """The one-forward stand-in for cross_check: one plain inference forward, ops.disparity_splat of its disparity -- the left
        map forward-warped into the right view, the nearest surface winning -- and ops.lr_check(disparity, splat, threshold, rel,
        mirrored=False).  Returns a CrossCheck: .disparity is bit-identical to forward's under torch.no_grad(), .disparity_right
        is the splatted plane (0 where nothing landed), .error, .kind and .filled are lr_check's.  The limits: every finite
        in-view pixel samples only columns it wrote to itself, so the interpolated r >= d, error = r - d >= 0 and kind 2
        (mismatch) never occurs; the check sees the occlusions that the left map's own geometry implies and cannot see a wrong
        match that the second forward would contradict; it marks up to one extra column at an occlusion edge, because the
        foreground claims both neighbours of its landing point; and nobody has measured its effect on EPE or D1."""
        return self._cross_check(left, right, threshold, rel, head, False, "splat")[0]

    def _cross_check(self, left, right, threshold, rel, head, with_source, check=None):
        """(the CrossCheck, src): cross_check's computation (check "cross") or self_check's ("splat"), the one occlusion_check
        names where check is None: what refine, despeckle and smooth pass; src [B,H,W] int32, the column each pixel of `filled`
        was copied from (its own where it is consistent, -1 for none), where with_source, else None."""
        check = _CHECK if check is None else check
        if isinstance(head, bool) or not isinstance(head, numbers.Integral) or not 0 <= head <= 2:     # before any device work
            raise ValueError(f"cross_check: head {head!r}: one of 0, 1, 2")
        threshold, rel = ops.check_lr_tolerances(threshold, rel)
        with torch.no_grad():
            out = self(left, right)[head]
            if out.dim() == 3:
                out = out.unsqueeze(1)
            if check == "splat":
                out_r = right_view = ops.disparity_splat(out).unsqueeze(1)
            else:
                out_r = self(torch.flip(right, (-1,)), torch.flip(left, (-1,)))[head].reshape(out.shape)
                right_view = torch.flip(out_r, (-1,))
            error, kind, filled, *src = ops.lr_check(out, out_r, threshold, rel, mirrored=check == "cross", with_source=with_source)
            cc = CrossCheck(out, right_view, error.unsqueeze(1), kind.unsqueeze(1), filled.unsqueeze(1))
            return cc, (src[0] if with_source else None)

    def refine(self, left, right, threshold=1.0, rel=0.0, head=2, median_radius=2, bilateral_radius=4, sigma_space=2.0,
               sigma_color=0.25):
        """cross_check, then the two image-space filters that make `filled` a dense map: ops.disparity_median (median_radius 1..3)
        over the pixels with filled > 0 -- one ATen compare; 0 is what a row without a consistent pixel holds -- and
        ops.disparity_bilateral (bilateral_radius, sigma_space in pixels, sigma_color in the units of `left`) of that median over
        the pixels with median > 0, guided by `left` as passed.  Returns a Refined: cross_check's five fields bit for bit, then
        .median and .refined, each [B,1,H,W].  median_radius=None skips the median (.median is .filled, and the bilateral reads
        it); bilateral_radius=None skips the bilateral (.refined is .median).  The defaults (5x5, 9x9, sigma 2 px, 0.25) are
        plausible values for images normalised as the model consumes them; their effect on EPE or D1 has not been measured.
        Inside an occlusion_check("splat") block it starts from self_check instead: one forward, with the limits stated there."""
        return self._refine(left, right, threshold, rel, head, median_radius, bilateral_radius, sigma_space, sigma_color, None, 1.0)

    def despeckle(self, left, right, threshold=1.0, rel=0.0, head=2, median_radius=2, bilateral_radius=4, sigma_space=2.0,
                  sigma_color=0.25, speckle_size=200, speckle_diff=1.0):
        """refine with the speckle filter in it, run where OpenCV's pipelines run it: on the checked map, before any filling.
        After cross_check, ops.disparity_speckle of .disparity over the consistent pixels (kind == 0) with max_size =
        speckle_size (an integer >= 0) and max_diff = speckle_diff; a pixel of `filled` then shares the fate of the pixel it was
        copied from (its own, where it is consistent): .despeckled is `filled` where that pixel's segment has more than
        speckle_size pixels and 0 elsewhere -- one gather along W and one where -- and refine's two filters read .despeckled in
        place of `filled` (valid = despeckled > 0; the None radii as in refine).  Returns a Despeckled: Refined's seven fields in
        the same order, the first five cross_check's bit for bit, then .despeckled and .segment (int32: the size of each pixel's
        segment, 0 where it is not consistent), each [B,1,H,W].  speckle_size=None is refine itself: the same code path, results
        and return type (speckle_diff is not looked at).  200 pixels and 1.0 are the values customary with OpenCV; their effect
        on EPE or D1 has not been measured either.  Inside an occlusion_check("splat") block it starts from self_check instead of
        cross_check (one forward, with the limits stated there)."""
        return self._refine(left, right, threshold, rel, head, median_radius, bilateral_radius, sigma_space, sigma_color,
                            speckle_size, speckle_diff)

    def _refine(self, left, right, threshold, rel, head, median_radius, bilateral_radius, sigma_space, sigma_color, speckle_size,
                speckle_diff):
        if median_radius is not None:                                                                  # before any device work
            median_radius = ops.check_median_radius(median_radius, "refine")
        if bilateral_radius is not None:
            bilateral_radius, sigma_space, sigma_color = ops.check_bilateral_parameters(bilateral_radius, sigma_space, sigma_color, "refine")
        if speckle_size is not None:
            speckle_size, speckle_diff = ops.check_speckle_parameters(speckle_size, speckle_diff, "despeckle")
        cc, src = self._cross_check(left, right, threshold, rel, head, speckle_size is not None)
        with torch.no_grad():
            median = cc.filled
            if speckle_size is not None:
                kept, _, segment = ops.disparity_speckle(cc.disparity, cc.kind == 0, speckle_size, speckle_diff, with_segments=True)
                source = torch.gather(kept, 2, src.clamp(min=0).long())                  # kept at the column the fill came from
                median = despeckled = torch.where((src >= 0) & (source > 0), cc.filled[:, 0], 0.0).unsqueeze(1)
            if median_radius is not None:
                median = ops.disparity_median(median, median > 0, median_radius).unsqueeze(1)
            refined = median
            if bilateral_radius is not None:
                refined = ops.disparity_bilateral(median, left, median > 0, bilateral_radius, sigma_space, sigma_color).unsqueeze(1)
            if speckle_size is not None:
                return Despeckled(*cc, median, refined, despeckled, segment.unsqueeze(1))
            return Refined(*cc, median, refined)

    def smooth(self, left, right, threshold=1.0, rel=0.0, head=2, speckle_size=200, speckle_diff=1.0, lam=8000.0, sigma_color=0.25,
               iterations=3):
        """cross_check, then the global smoother that ends OpenCV's chain (DisparityWLSFilter), in place of every local fill:
        with speckle_size not None, ops.disparity_speckle of .disparity over the consistent pixels exactly as despeckle runs it;
        confidence = 1.0 where kind == 0 and (speckles on) the pixel's segment has more than speckle_size pixels, else 0; then
        ops.disparity_wls(.disparity, left, confidence, lam, sigma_color, iterations), guided by `left` as passed.  Neither
        `filled`, the median nor the bilateral filter is run: a hole is a pixel of confidence 0 and is written from as far away as
        the guide's edges allow.  Returns a Smoothed: cross_check's five fields bit for bit, then .confidence and .smoothed, each
        [B,1,H,W].  The defaults are untested for quality: 8000 and 3 are the values customary with OpenCV, 0.25 is the bilateral
        filter's default in the units of `left`, 200 and 1.0 are despeckle's; nobody has measured their effect on EPE or D1.
        Inside an occlusion_check("splat") block it starts from self_check instead of cross_check (one forward, with the limits
        stated there)."""
        lam, sigma_color, iterations = ops.check_wls_parameters(lam, sigma_color, iterations, "smooth")  # before any device work
        if speckle_size is not None:
            speckle_size, speckle_diff = ops.check_speckle_parameters(speckle_size, speckle_diff, "smooth")
        cc, _ = self._cross_check(left, right, threshold, rel, head, False)
        with torch.no_grad():
            confident = cc.kind == 0
            if speckle_size is not None:
                _, _, segment = ops.disparity_speckle(cc.disparity, confident, speckle_size, speckle_diff, with_segments=True)
                confident = confident & (segment.unsqueeze(1) > speckle_size)
            confidence = confident.to(torch.float32)
            smoothed = ops.disparity_wls(cc.disparity, left, confidence, lam, sigma_color, iterations).unsqueeze(1)
            return Smoothed(*cc, confidence, smoothed)

    def point_cloud(self, left, right, Q, colors=None, source="smooth", min_disp=0.0, max_disp=None, **stage_args):
        """From the image pair to geometry: the entry point named by `source` -- "forward", "self_check", "cross_check", "refine",
        "despeckle" or "smooth", called with stage_args -- then ops.point_cloud of its final plane (head 2 of forward; .filled,
        .refined or .smoothed of the others) with the matrix Q (ops.q_matrix), over the pixels where that plane is > 0 (every
        pixel for "forward"; a hole of the chains is 0) and min_disp < d <= max_disp.  colors ([B,C,H,W] fp32, C <= 4; None: no
        attributes; `left` gives XYZRGB rows in the normalisation the model consumes) is gathered beside the coordinates.
        Returns a PointCloud: .points [N, 3 + C], .offsets [B + 1], .xyz [B,3,H,W], .mask [B,H,W] and .stage, the entry point's
        own result bit for bit.  It calls the same methods, so an occlusion_check("splat") block applies; it needs `forward`
        only, so every registered architecture has it.  An unknown source, a bad Q or bound raises ValueError before any device
        work.  The defaults say nothing about EPE or D1, and Q's sign conventions are the caller's."""
        if not isinstance(source, str) or source not in POINT_CLOUD_SOURCES:                          # before any device work
            raise ValueError(f"point_cloud: source {source!r}: one of {tuple(POINT_CLOUD_SOURCES)}")
        n_colors = colors.shape[1] if isinstance(colors, torch.Tensor) and colors.dim() == 4 else 0
        ops.check_reproject_parameters(Q, min_disp, max_disp, n_colors, "point_cloud")
        with torch.no_grad():
            if source == "forward":
                stage = self(left, right, **stage_args)
                plane, valid = stage[2], None
            else:
                stage = getattr(self, source)(left, right, **stage_args)
                plane = getattr(stage, POINT_CLOUD_SOURCES[source])
                valid = plane > 0
            return PointCloud(*ops.point_cloud(plane, Q, colors, valid, min_disp, max_disp, with_dense=True), stage)


class cmfsm(_ECMNet):
    """cmfsm.py:594-774.  forward(left, right) -> (pred1, pred2, pred3), each [B,1,H,W] in pixels."""
    ENCODER, HOURGLASSES, HEAD, PRE1_FORK = "cmfsm", 3, "eight", True
    LEVEL_SPACING = 4      # the levels are the low-resolution disparities; eight_related_context_mapping exists at scale 4 only

    def hot_path(self, lr_l, hr_l, lr_r):
        """Everything after the encoder (cmfsm.py:659-774)."""
        scale = hr_l.shape[-1] // lr_l.shape[-1]
        w9 = self.mapping_matrix.weights(lr_l, hr_l)                                   # :664
        heads = self._aggregate(lr_l, lr_r, self.maxdisp // scale)                     # :667-693, 695, 724, 747
        disp = ops.softargmin_heads(torch.stack(heads, 0))                             # :703-706,725-728,748-753
        preds = ops.ecm_aggregate9(disp, w9, scale)                                    # :709-723 (x3)
        return preds[0].unsqueeze(1), preds[1].unsqueeze(1), preds[2].unsqueeze(1)

    def forward(self, left, right):
        # cmfsm.py:657-658 runs the shared encoder twice; both images go through it as ONE batch here (GroupNorm has no
        # cross-sample statistics, so the result is identical) -- half the launches, better-filled small layers.
        B = left.shape[0]
        if torch.is_grad_enabled():
            ops.pace_side_streams()        # host run-ahead bound: the previous step's side-stream weight gradients have finished
        lr, _, hr = self.feature_extraction(torch.cat([left, right], 0), head=B)      # hr: the left images' map only
        return self.hot_path(lr[:B], hr, lr[B:])

    def head_stats(self, left, right):
        B = left.shape[0]
        lr, _, hr = self.feature_extraction(torch.cat([left, right], 0), head=B)
        lr_l, lr_r = lr[:B], lr[B:]
        scale = hr.shape[-1] // lr_l.shape[-1]
        w9 = self.mapping_matrix.weights(lr_l, hr)
        args = (torch.stack(self._aggregate(lr_l, lr_r, self.maxdisp // scale), 0), w9, scale)
        return ops.ecm_aggregate9_stats(*args), args


class cmfsm_sub_8(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub8", 3, "five"


class cmfsm_sub_16(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub16", 3, "volume"


class cm_sub_4(_ECMNet):
    ENCODER, HOURGLASSES, HEAD, SIM2 = "sub4", 1, "volume", True


class cm_sub_8(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub8", 1, "volume"


class cm_sub_16(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub16", 1, "volume"


class bilinear_cmf(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub4", 3, "trilinear"


class bilinear_cmf_sub_8(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub8", 3, "trilinear"


class bilinear_cmf_sub_16(_ECMNet):
    ENCODER, HOURGLASSES, HEAD = "sub16", 3, "trilinear"


# ------------------------------------------------------------------------------------------------
# cmf: super-resolution refinement decoder (cmf.py:227-264)
# ------------------------------------------------------------------------------------------------
class HipConvTranspose2d(nn.ConvTranspose2d):
    """nn.ConvTranspose2d(Ci, Co, 3, stride 2, pad 1, output_padding 1, bias=True) of the decoder (cmf.py:236-239) on the
    bias-taking 2-D transposed-convolution kernel (ops.deconv2d_k3s2_bias); any other configuration raises unless
    ECM_ALLOW_FALLBACK=1 (like EncConv2d)."""

    def _native(self):
        return (self.kernel_size == (3, 3) and self.stride == (2, 2) and self.padding == (1, 1)
                and self.output_padding == (1, 1) and self.dilation == (1, 1) and self.groups == 1 and self.bias is not None
                and self.padding_mode == "zeros" and self.out_channels <= 64 and self.in_channels % 4 == 0)

    def forward(self, x, output_size=None):
        if x.dtype == torch.bfloat16:                      # the bf16 decoder (ops.decoder_dtype)
            if not (self._native() and output_size is None and ops.deconv2d_bf16_supported(self.in_channels, self.out_channels)):
                raise RuntimeError(f"HipConvTranspose2d({self.in_channels}->{self.out_channels}, k={self.kernel_size}, "
                                   f"s={self.stride}) is outside the bf16 decoder kernel (ops.deconv2d_bf16_supported); leave the "
                                   "decoder_dtype(torch.bfloat16) block")
            return ops.deconv2d_k3s2_bias_bf16(x, self.weight, self.bias)
        if self._native() and output_size is None:
            return ops.deconv2d_k3s2_bias(x, self.weight, self.bias)
        if not ALLOW_FALLBACK:
            raise RuntimeError(f"HipConvTranspose2d({self.in_channels}->{self.out_channels}, k={self.kernel_size}, s={self.stride}, "
                               f"p={self.padding}, op={self.output_padding}, bias={self.bias is not None}) is outside the native "
                               "kernels; set ECM_ALLOW_FALLBACK=1 to run it on PyTorch-ROCm's own convolution instead")
        SLOW_PATH_EVENTS.append(("miopen_conv_transpose2d", self.in_channels, self.out_channels, self.kernel_size))
        return super().forward(x, output_size)


class HipConv2dC1(nn.Conv2d):
    """conv_out, nn.Conv2d(96, 1, 3, 1, 1, bias=True) (cmf.py:259), with the ReLU that follows it (`crap`, cmf.py:260,264)
    fused: forward() returns relu(conv(x)) on the one-output-channel kernels (ops.conv2d_c1_relu)."""

    def _native(self):
        return (self.out_channels == 1 and self.kernel_size == (3, 3) and self.stride == (1, 1) and self.padding == (1, 1)
                and self.dilation == (1, 1) and self.groups == 1 and self.bias is not None and self.padding_mode == "zeros")

    def forward(self, x):
        if x.dtype == torch.bfloat16:                      # the bf16 decoder (ops.decoder_dtype): fp32 result
            if not (self._native() and self.in_channels % 16 == 0):
                raise RuntimeError(f"HipConv2dC1({self.in_channels}->{self.out_channels}, k={self.kernel_size}) is outside the "
                                   "bf16 decoder kernel; leave the decoder_dtype(torch.bfloat16) block")
            return ops.conv2d_c1_relu_bf16(x, self.weight, self.bias)
        if self._native():
            return ops.conv2d_c1_relu(x, self.weight, self.bias)
        if not ALLOW_FALLBACK:
            raise RuntimeError(f"HipConv2dC1({self.in_channels}->{self.out_channels}, k={self.kernel_size}) is outside the native "
                               "kernels; set ECM_ALLOW_FALLBACK=1 to run it on PyTorch-ROCm's own convolution instead")
        SLOW_PATH_EVENTS.append(("miopen_conv2d", self.in_channels, self.out_channels, self.kernel_size))
        return F.relu(super().forward(x))


def _cat_shared(x, shared, nh):
    """cat([x, shared repeated over the nh heads], 1) for x [nh*B,C,h,w] and shared [B,C',h,w]: the shared map enters as an
    expanded view (the cat writes those channels anyway); autograd sums its nh gradients in a fixed order."""
    B = shared.shape[0]
    x5 = x.view(nh, B, *x.shape[1:])
    return torch.cat([x5, shared.unsqueeze(0).expand(nh, *shared.shape)], 2).view(nh * B, -1, *x.shape[-2:])


class super_resolution_refinement(nn.Module):
    """cmf.py:227-264.  forward(preds [NH,B,h,w], rgb [B,3,4h,4w], refimg_fea [B,32,h,w], half [B,32,2h,2w]) ->
    [NH,B,1,4h,4w].  The reference calls the module once per head with the same rgb / features (cmf.py:437,442,447); here the
    NH heads are ONE pass over an NH*B batch (shared weights, per-sample GroupNorm: the same result), rgb_fea(rgb) is
    computed once, and the shared maps join the concatenations as expanded views."""

    def __init__(self, dis_planes=32, twice_times=2):
        super().__init__()
        self.twice_times = twice_times
        self.conv1 = nn.Sequential(convbn(1, dis_planes * 2, 3, 1, 1, 1), nn.ReLU(inplace=True))
        self.deconv_module_list = nn.ModuleList([nn.Sequential(
            HipConvTranspose2d(dis_planes * 3, dis_planes * 2, 3, 2, 1, 1),
            HipGroupNorm(NUM_GROUPS, dis_planes * 2), nn.ReLU(inplace=True)) for _ in range(twice_times)])
        self.rgb_fea = nn.Sequential(
            convbn(3, dis_planes, 3, 1, 1, 1), nn.ReLU(inplace=True),
            convbn(dis_planes, dis_planes, 3, 1, 1, 1), nn.ReLU(inplace=True),
            convbn(dis_planes, dis_planes, 3, 1, 1, 1), nn.ReLU(inplace=True))
        self.conv2 = nn.Sequential(convbn(dis_planes * 3, dis_planes * 3, 3, 1, 1, 1), nn.ReLU(inplace=True))
        self.conv_out = HipConv2dC1(dis_planes * 3, 1, 3, 1, 1)
        self.crap = HipReLU(inplace=True)                  # fused into conv_out

    def forward(self, preds, rgb, *rgb_zoom_feature):
        """Inside ops.decoder_dtype(torch.bfloat16): _forward_bf16."""
        bf16 = ops.decoder_bf16()
        if bf16:
            ops._DEC.no_grad("super_resolution_refinement")         # before the first launch
        if len(rgb_zoom_feature) != self.twice_times:
            raise ValueError(f"super_resolution_refinement: {self.twice_times} zoom features expected, got {len(rgb_zoom_feature)}")
        NH, B, h, w = preds.shape
        f = 2 ** self.twice_times
        want = [(B, h * 2 ** i, w * 2 ** i) for i in range(self.twice_times)]
        got = [(t.shape[0], t.shape[-2], t.shape[-1]) for t in rgb_zoom_feature]
        if got != want or rgb.shape[0] != B or tuple(rgb.shape[-2:]) != (h * f, w * f):
            raise ValueError(f"super_resolution_refinement: preds {tuple(preds.shape)}, rgb {tuple(rgb.shape)}, zoom features "
                             f"{[tuple(t.shape) for t in rgb_zoom_feature]}: each map must be twice the size of the previous one")
        if bf16:
            return self._forward_bf16(preds, rgb, rgb_zoom_feature)
        x = _seq_fused(self.conv1, preds.reshape(NH * B, 1, h, w))                 # cmf.py:258
        for dec, skip in zip(self.deconv_module_list, rgb_zoom_feature):            # cmf.py:259-260
            x = dec[1].fused(dec[0](_cat_shared(x, skip, NH)), None, True)
        x = _cat_shared(x, _seq_fused(self.rgb_fea, rgb), NH)                      # cmf.py:262
        x = self.conv_out(_seq_fused(self.conv2, x))                               # cmf.py:263-264 (+ crap)
        return x.view(NH, B, 1, h * f, w * f)

    def _forward_bf16(self, preds, rgb, rgb_zoom_feature):
        """The decoder on bf16 maps (ops.decoder_dtype).  fp32 enters where rounding would hurt: conv1 reads the fp32
        disparities (values up to maxdisp/4: 8 bits would not hold them) and rgb_fea's stem the fp32 image, both on the fp32
        kernels, and their GroupNorm + ReLU writes bf16.  The encoder maps that join the concatenations are rounded once.
        Every later layer runs on the bf16 kernels (a layer outside them raises): the transposed convolutions and conv_out on
        bf16_decoder.hip, rgb_fea's 32 -> 32 layers and conv2 on the encoder's convolution kernel, the GroupNorms on the
        two-stage kernels.  The result is fp32, written by conv_out's kernel."""
        bf = torch.bfloat16
        NH, B, h, w = preds.shape
        f = 2 ** self.twice_times
        conv, gn = self.conv1[0][0], self.conv1[0][1]
        x = gn.fused(conv(preds.reshape(NH * B, 1, h, w)), None, True, out_dtype=bf)
        for dec, skip in zip(self.deconv_module_list, rgb_zoom_feature):
            x = dec[1].fused(dec[0](_cat_shared(x, skip.to(bf), NH)), None, True)
        conv, gn = self.rgb_fea[0][0], self.rgb_fea[0][1]
        r = _seq_fused(self.rgb_fea, gn.fused(conv(rgb), None, True, out_dtype=bf), start=2)
        x = self.conv_out(_seq_fused(self.conv2, _cat_shared(x, r, NH)))
        return x.view(NH, B, 1, h * f, w * f)


class cmf(_ECMNet):
    """cmf.py:267-450.  forward(left, right) -> (pred1, pred2, pred3), each [B,1,H,W]: the cmfsm 3-D stack and accumulated
    soft-argmin heads on the 1/4-resolution cost volume, each head's quarter-resolution disparity refined to full resolution by
    the shared super_resolution_refinement decoder.  H and W must be multiples of 4 (the decoder doubles 1/4 -> 1/2 -> 1)."""
    ENCODER, HOURGLASSES, HEAD = "cmf", 3, "srr"

    def __init__(self, maxdisp=192):
        super().__init__(maxdisp)
        self.srr = super_resolution_refinement(32, 2)
        for m in self.srr.modules():                                   # cmf.py:377-392 (ConvTranspose2d and biases: default)
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))

    def hot_path(self, lr_l, lr_r, left, half):
        """Cost volume -> dres0/1 -> three hourglasses -> accumulated heads (cmf.py:394-436) -> decoder (cmf.py:437-449)."""
        heads = self._aggregate(lr_l, lr_r, self.maxdisp // 4)         # dres4(out2, pre1, post2): cmf.py:413
        disp = ops.softargmin_heads(torch.stack(heads, 0))            # [3,B,h,w], quarter-resolution units
        preds = self.srr(disp, left, lr_l, half)
        return preds[0], preds[1], preds[2]

    def forward(self, left, right):
        H, W = left.shape[-2:]
        if H % 4 or W % 4 or tuple(right.shape) != tuple(left.shape):
            raise ValueError(f"cmf: left {tuple(left.shape)}, right {tuple(right.shape)}: H and W must be multiples of 4 (the "
                             "decoder doubles 1/4 -> 1/2 -> 1) and both images the same size")
        B = left.shape[0]
        ops._DEC.guard("cmf")                                          # the bf16 decoder has no backward: raise before any launch
        if torch.is_grad_enabled():
            ops.pace_side_streams()
        lr, _, half = self.feature_extraction(torch.cat([left, right], 0), head=B)   # one encoder pass for both images
        return self.hot_path(lr[:B], lr[B:], left, half)


_MODELS = {"cmfsm": cmfsm, "cmfsm_sub_8": cmfsm_sub_8, "cmfsm_sub_16": cmfsm_sub_16, "cm_sub_4": cm_sub_4,
           "cm_sub_8": cm_sub_8, "cm_sub_16": cm_sub_16, "bilinear_cmf": bilinear_cmf,
           "bilinear_cmf_sub_8": bilinear_cmf_sub_8, "bilinear_cmf_sub_16": bilinear_cmf_sub_16, "cmf": cmf}


def get_model(name):
    """cmf/models/__init__.py:19-41: returns `cls()`; an unknown name prints and returns None like the reference."""
    cls = _MODELS.get(name)
    if cls is None:
        print("Model {} not available".format(name))
        return None
    return cls()


class StereoRig:
    """A calibrated horizontal rig: from raw, distorted camera frames to the inputs of the network and, with
    a model, to a metric point cloud, without leaving the device.  A plain object, not a module: .rectification is
    ops.stereo_rectify's result for (K1, D1, K2, D2, R, T, size, new_size, focal, center), .Q its disparity-to-depth matrix
    (what ops.disparity_reproject and _ECMNet.point_cloud take).  No model method is added or changed."""

    def __init__(self, K1, D1, K2, D2, R, T, size, new_size=None, focal=None, center=None):
        self.rectification = ops.stereo_rectify(K1, D1, K2, D2, R, T, size, new_size, focal, center)
        self.Q = self.rectification.Q
        self._cameras = ((K1.detach().clone(), D1.detach().clone()), (K2.detach().clone(), D2.detach().clone()))
        self._maps = {}

    def maps(self, device):
        """(map_left, map_right), each [2,Ho,Wo] fp32 on `device`: ops.rectify_map of each camera, computed once per device."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._maps:
            r = self.rectification
            self._maps[device] = tuple(ops.rectify_map(K, D, Rn, Pn, r.new_size, device)
                                       for (K, D), Rn, Pn in zip(self._cameras, (r.R1, r.R2), (r.P1, r.P2)))
        return self._maps[device]

    def __call__(self, left_raw, right_raw, want_image=False, with_mask=False):
        """ops.remap_pair of the raw pair (uint8 [B,H,W,3] or float32 [B,3,H,W] of the calibrated size) through this rig's maps:
        (left, right[, image][, mask_left, mask_right])."""
        if not isinstance(left_raw, torch.Tensor) or not left_raw.is_cuda:
            raise RuntimeError("ecm ops run only on the MI355X HIP path: got a CPU tensor (no CPU fallback exists)")
        hw = tuple(left_raw.shape[1:3]) if left_raw.dtype == torch.uint8 else tuple(left_raw.shape[2:4])
        if left_raw.dim() != 4 or hw != self.rectification.size:
            raise ValueError(f"StereoRig: frames {tuple(left_raw.shape)}: the rig was calibrated at (H, W) = {self.rectification.size}")
        map_left, map_right = self.maps(left_raw.device)
        return ops.remap_pair(left_raw, right_raw, map_left, map_right, want_image=want_image, with_mask=with_mask)

    def point_cloud(self, model, left_raw, right_raw, source="smooth", colors="image", **stage_args):
        """Rectify the raw pair, then model.point_cloud(left, right, self.Q, colors=..., source=source, **stage_args): that
        PointCloud, unchanged.  colors: "image" (the rectified left image in /255 units: XYZRGB rows), None, or a tensor
        [B,C,Ho,Wo] of the caller's."""
        if isinstance(colors, str) and colors != "image":
            raise ValueError(f"StereoRig.point_cloud: colors {colors!r}: \"image\", None or a tensor")
        if isinstance(colors, str):
            left, right, colors = self(left_raw, right_raw, want_image=True)
        else:
            left, right = self(left_raw, right_raw)
        return model.point_cloud(left, right, self.Q, colors=colors, source=source, **stage_args)


# What DisparityTracker returns, each field [B,1,H,W]: this frame's own disparity and std, bit for bit; the
# previous state warped into this frame (zeros where it starts over); and the new state: the fused disparity, its variance and
# the number of frames it has been measured over (int32).
Tracked = collections.namedtuple("Tracked", "disparity std warped fused variance age")


class DisparityTracker:
    """Disparity carried from frame to frame by the camera's known motion: per call one model.predict for
    the disparity and std of `head` (for the architectures whose predict raises NotImplementedError, one plain forward and the
    constant std sigma0), ops.disparity_warp of the state by ops.warp_matrix(Q, motion) with the planes (variance, disparity, age)
    as attributes -- age travels as a float plane, exact below 2^24 -- and ops.disparity_fuse(disparity, std^2, warped state,
    gate, process_noise, coast) with the pre-warp disparity as prev_source; (fused, variance, age) is the next call's state.
    motion (float64 CPU [4,4] or [B,4,4]) takes points of the previous left-camera frame to this one, in the unit of Q's baseline;
    motion=None, a first call, a changed shape and reset() start over: warped is zeros and the state is this frame's own.  A plain
    object without parameters, not a module; it changes nothing in the model.  A static-scene model: a moving object is caught by
    the gate alone; "cover" thickens foreground edges by up to a pixel; the defaults of gate, process_noise and sigma0 are
    untested for quality, and nobody has measured the effect on EPE, D1 or temporal stability."""

    def __init__(self, model, Q, head=2, gate=3.0, process_noise=0.01, sigma0=1.0, footprint="cover", coast=True):
        if not isinstance(model, _ECMNet):
            raise ValueError(f"DisparityTracker: model {type(model).__name__}: one of the registered architectures")
        if isinstance(head, bool) or not isinstance(head, numbers.Integral) or not 0 <= head <= 2:
            raise ValueError(f"DisparityTracker: head {head!r}: one of 0, 1, 2")
        ops.warp_matrix(Q, torch.eye(4, dtype=torch.float64))              # Q's own refusals, a singular Q among them
        self.gate, self.process_noise, _ = ops.check_fuse_parameters(gate, process_noise, coast, "DisparityTracker")
        self.sigma0 = ops._real("DisparityTracker", "sigma0", sigma0, "> 0", fp32=True)
        if footprint not in ops.WARP_FOOTPRINTS:
            raise ValueError(f"DisparityTracker: footprint {footprint!r}: one of {ops.WARP_FOOTPRINTS}")
        self.model, self.Q, self.head, self.footprint, self.coast = model, Q.detach().clone(), int(head), footprint, coast
        self._state = None

    def reset(self):
        """Forget the state: the next call starts over."""
        self._state = None

    def measure(self, left, right):
        """The measuring half of a call: this frame's own (disparity, std), each [B,1,H,W]; the state is not touched."""
        with torch.no_grad():
            if self.model.HEAD in _NO_DISTRIBUTION:
                disparity = self.model(left, right)[self.head]
                if disparity.dim() == 3:
                    disparity = disparity.unsqueeze(1)
                std = torch.full_like(disparity, self.sigma0)
            else:
                p = self.model.predict(left, right, (self.head,))
                disparity, std = p.disparity[0], p.std[0]
        return disparity, std

    def carries(self, disparity):
        """Whether the state can be carried into a frame whose disparity is `disparity`: it exists, with that shape and device."""
        state = self._state
        return state is not None and state[0].shape == disparity.shape and state[0].device == disparity.device

    def advance(self, disparity, std, M):
        """The advancing half of a call: the state warped by M (None: start over) and fused with the measurement; the Tracked."""
        with torch.no_grad():
            if M is None or not self.carries(disparity):
                warped, prev_var, prev_source = (torch.zeros_like(disparity) for _ in range(3))
                prev_age = torch.zeros_like(disparity, dtype=torch.int32)
            else:
                fused, variance, age = self._state
                warped, carried = ops.disparity_warp(fused, M, attributes=torch.cat([variance, fused, age.to(torch.float32)], 1),
                                                     footprint=self.footprint)
                prev_var, prev_source, prev_age = carried[:, 0:1], carried[:, 1:2], carried[:, 2:3].to(torch.int32)
            self._state = ops.disparity_fuse(disparity, std * std, warped, prev_var, prev_age, prev_source, self.gate,
                                             self.process_noise, self.coast)
        return Tracked(disparity, std, warped, *self._state)

    def __call__(self, left, right, motion=None):
        M = None if motion is None else ops.warp_matrix(self.Q, motion)    # ValueError before any device work
        return self.advance(*self.measure(left, right), M)


# What StereoOdometry returns: Tracked's six fields as DisparityTracker returns them for `motion`; motion [B,4,4] float64 CPU, the
# estimated motion from the previous frame to this one (the identity where the frame starts over); pose [B,4,4], the product of
# the motions since the last start, so that it takes points of the starting frame to this one; estimate, the ops.MotionEstimate
# (None where there was no state to align to); restarted: the frame started over (a first call, a reset, a changed shape, or an
# estimate that did not converge for some image of the batch).
Odometry = collections.namedtuple("Odometry", Tracked._fields + ("motion", "pose", "estimate", "restarted"))


class StereoOdometry:
    """DisparityTracker for a rig whose motion is NOT known: per call the frame's predict
    (DisparityTracker.measure), ops.motion_estimate from the carried state to this frame's disparity -- disp0 the fused state
    with valid0 = fused > 0 and weight = 1 / variance, init the previous frame's motion (constant velocity), on the lattice of
    `step` -- and the tracker's warp and fuse (DisparityTracker.advance) with the estimate.  Where the estimate does not
    converge for every image of the batch the frame starts over as motion=None does, and `restarted` says so.  A plain object
    like the tracker; reset() forgets the state, the velocity and the pose.  A static-scene estimator without a pyramid; every
    default is untested for quality, and nobody has measured it on real sequences."""

    def __init__(self, model, Q, head=2, step=2, iterations=10, damping=1e-6, tolerance=1e-7, min_pixels=64, tap_range=1.0,
                 max_residual=3.0, cauchy=1.0, gate=3.0, process_noise=0.01, sigma0=1.0, footprint="cover", coast=True):
        self.tracker = DisparityTracker(model, Q, head, gate, process_noise, sigma0, footprint, coast)
        eye = torch.eye(4, dtype=torch.float64)
        ops._align_matrices("StereoOdometry", Q, eye, None)               # the estimator's own refusals, before any frame is seen
        ops.check_align_parameters(step, 0.0, None, tap_range, max_residual, cauchy, "StereoOdometry")
        ops.check_estimate_parameters(iterations, damping, tolerance, min_pixels, "StereoOdometry")
        self.estimator = dict(step=step, iterations=iterations, damping=damping, tolerance=tolerance, min_pixels=min_pixels,
                              tap_range=tap_range, max_residual=max_residual, cauchy=cauchy)
        self.Q = self.tracker.Q
        self._velocity, self._pose, self._eye = None, None, eye

    def reset(self):
        """Forget the state, the velocity and the pose: the next call starts over."""
        self.tracker.reset()
        self._velocity = self._pose = None

    def __call__(self, left, right):
        disparity, std = self.tracker.measure(left, right)
        B = disparity.shape[0]
        estimate, motion = None, None
        if self.tracker.carries(disparity):
            fused, variance, _ = self.tracker._state
            init = self._velocity if self._velocity is not None and self._velocity.shape[0] == B else None
            with torch.no_grad():
                estimate = ops.motion_estimate(fused, disparity, self.Q, init, valid0=fused > 0, weight=1.0 / variance,
                                               **self.estimator)
            if bool(estimate.converged.all()):
                motion = estimate.T
        restarted = motion is None
        tracked = self.tracker.advance(disparity, std, None if restarted else ops.warp_matrix(self.Q, motion))
        if restarted:
            motion = self._eye.expand(B, 4, 4).clone()
            self._velocity, self._pose = None, motion.clone()
        else:
            self._velocity, self._pose = motion, motion @ self._pose
        return Odometry(*tracked, motion, self._pose.clone(), estimate, restarted)


# What StereoMapper returns: Odometry's ten fields as the odometry (or, for a given motion, the tracker) returns them, bit for bit;
# world [4,4] float64 CPU, the pose of this frame's left camera (it takes points of the first frame's left-camera frame, the
# world frame, to this one); integrated: the frame went into the volume; frames: the frames integrated since the last reset.
Mapped = collections.namedtuple("Mapped", Odometry._fields + ("world", "integrated", "frames"))


class StereoMapper:
    """A TSDF volume filled by a moving stereo rig: per call one StereoOdometry frame -- or, where the
    motion from the previous frame is known (`motion`, as DisparityTracker takes it), one frame of the odometry's tracker -- the
    update world = motion @ world of the mapper's own pose, and ops.volume_integrate of the frame's OWN disparity at that pose
    with weight = 1 / std^2 and valid = disparity > 0 (not the fused state, whose history the volume would count twice).  The
    world frame is the first frame's left camera; the volume has dims = (nz, ny, nx) voxels of `voxel` (the unit of Q's baseline)
    from `origin`, and is allocated on the first frame's device.  A frame after the first whose estimate did not converge
    (Odometry.restarted) is not integrated and the pose is held: what follows is placed as if the rig had not moved over it.
    render() raycasts the volume at the current pose or a given one; mesh() extracts its surface as a triangle mesh; reset()
    empties the volume and forgets the poses.  A plain
    object, not a module; batch size 1.  A static-scene model with a dense volume; the distance is along the optical axis, the
    weight ignores that depth noise grows with Z^2 (min_disp is the guard against far, noisy pixels); every default is untested
    for quality, and nobody has measured it on real sequences."""

    def __init__(self, model, Q, origin, voxel, dims, trunc, head=2, max_weight=64.0, min_disp=1.0, **odometry_kwargs):
        self.odometry = StereoOdometry(model, Q, head, **odometry_kwargs)
        self.Q = self.odometry.Q
        eye = torch.eye(4, dtype=torch.float64)
        ops.volume_matrices(self.Q, eye, origin, voxel)                   # origin, voxel and a singular Q, before any frame is seen
        self.dims = ops._volume_dims("StereoMapper", dims)
        ops.check_volume_parameters(trunc, max_weight, min_disp, None, "StereoMapper")
        self.origin, self.voxel, self.trunc, self.max_weight, self.min_disp = origin, voxel, trunc, max_weight, min_disp
        self.volume, self.world, self.frames, self._size, self._eye = None, eye.clone(), 0, None, eye

    def reset(self):
        """Empty the volume and forget the poses and the tracker's state: the next frame defines the world frame."""
        self.odometry.reset()
        if self.volume is not None:
            self.volume[0].fill_(1.0)
            self.volume[1].zero_()
        self.world, self.frames = self._eye.clone(), 0

    def _allocate(self, device):
        """The empty volume on `device`."""
        self.volume = ops.volume_new(self.dims, device)

    def _frame_kwargs(self, o):
        """How a frame (an Odometry) counts in the volume, as keyword arguments of the integrate ops."""
        return dict(valid=o.disparity > 0, weight=1.0 / (o.std * o.std), max_weight=self.max_weight, min_disp=self.min_disp)

    def _integrate(self, o, extra=None):
        """One frame (an Odometry) into the volume at the pose self.world; `extra` is what a subclass's __call__ passed on."""
        ops.volume_integrate(*self.volume, o.disparity, self.Q, self.world, self.origin, self.voxel, self.trunc, **self._frame_kwargs(o))

    def __call__(self, left, right, motion=None):
        return self._frame(left, right, motion)

    def _frame(self, left, right, motion, extra=None):
        if not isinstance(left, torch.Tensor) or left.dim() != 4 or left.shape[0] != 1:
            raise ValueError(f"StereoMapper: frames {tuple(getattr(left, 'shape', ()))}: one pair at a time, [1,3,H,W]")
        first = self.frames == 0
        if motion is None:
            o = self.odometry(left, right)
            moved, held = o.motion[0], o.restarted and not first
        else:
            M = ops.warp_matrix(self.Q, motion)                           # ValueError before any device work
            motion = motion if motion.dim() == 3 else motion.unsqueeze(0)
            if motion.shape[0] != 1:
                raise ValueError(f"StereoMapper: motion {tuple(motion.shape)}: one pair at a time")
            tracker = self.odometry.tracker
            disparity, std = tracker.measure(left, right)
            carried = tracker.carries(disparity)
            tracked = tracker.advance(disparity, std, M)
            moved, held = motion[0], False
            o = Odometry(*tracked, motion.clone(), (self._eye if first else moved @ self.world)[None].clone(), None, not carried)
        if not (first or held):
            self.world = moved @ self.world
        if self.volume is None or self.volume[0].device != o.disparity.device:
            self._allocate(o.disparity.device)
        self._size = tuple(o.disparity.shape[-2:])
        if not held:
            with torch.no_grad():
                self._integrate(o, extra)
            self.frames += 1
        return Mapped(*o, self.world.clone(), not held, self.frames)

    def render(self, T=None, size=None, near_disp=None, far_disp=None, step=0.5, max_steps=None, with_weight=False, Q_out=None):
        """ops.volume_raycast of the volume at the current pose (T None) or at T (world to camera), for the view Q_out (None: Q)
        of size (H, W) (None: the last frame's): near_disp None is W, the largest disparity a map of that width can hold, and
        far_disp None is min_disp."""
        view = self._view("StereoMapper.render", T, size, near_disp, far_disp, Q_out)
        return ops.volume_raycast(*self.volume, *view, step, max_steps, with_weight)

    def _need_frames(self, who):
        if self.volume is None:
            raise ValueError(f"{who}: no frame has been integrated")

    def _view(self, who, T, size, near_disp, far_disp, Q_out):
        """render()'s guard and defaults: (Q_out, T, origin, voxel, size, near_disp, far_disp) as the raycast ops take them."""
        self._need_frames(who)
        size = self._size if size is None else size
        near_disp = float(size[1]) if near_disp is None and isinstance(size, (tuple, list)) and len(size) == 2 else near_disp
        return (self.Q if Q_out is None else Q_out, self.world if T is None else T, self.origin, self.voxel, size, near_disp,
                self.min_disp if far_disp is None else far_disp)

    def mesh(self, min_weight=0.0, **kw):
        """mesh.volume_mesh of the volume in the world frame (the first frame's left camera): Mesh(vertices, faces, normals,
        weight); kw: with_normals, with_weight, or T for another camera's frame."""
        self._need_frames("StereoMapper.mesh")
        return _mesh.volume_mesh(*self.volume, self.origin, self.voxel, min_weight=min_weight, **kw)


class ColorStereoMapper(StereoMapper):
    """A StereoMapper whose volume also carries `channels` attribute planes: per call the frame's colours
    -- `colors` [1,channels,H,W] fp32 of the disparity's size, or the left image as given (None; it has three channels) -- go
    into the volume with the frame's disparity through color.volume_integrate, one launch in ops.volume_integrate's place, so
    the Mapped it returns, tsdf and wsum are a plain StereoMapper's bit for bit.  render_colors() raycasts disparity and colour,
    colored_mesh() extracts the mesh and samples the colour at its vertices; render() and mesh() are StereoMapper's.  The
    attributes are averaged as they are given (a normalised image stays normalised: the caller de-normalises what it reads
    back).  The colour band is trunc wide, a voxel reads the nearest pixel, and there is no view-angle weighting; every
    default is untested for quality, and only synthetic scenes were used."""

    def __init__(self, model, Q, origin, voxel, dims, trunc, head=2, max_weight=64.0, min_disp=1.0, channels=3, **odometry_kwargs):
        super().__init__(model, Q, origin, voxel, dims, trunc, head, max_weight, min_disp, **odometry_kwargs)
        self.channels = _color._channels("ColorStereoMapper", channels)
        self.attributes = None

    def reset(self):
        """StereoMapper.reset(), and the attribute planes emptied too."""
        super().reset()
        if self.attributes is not None:
            self.attributes[0].zero_()
            self.attributes[1].zero_()

    def _allocate(self, device):
        super()._allocate(device)
        self.attributes = _color.volume_attributes_new(self.dims, self.channels, device)

    def _integrate(self, o, extra=None):
        _color.volume_integrate(*self.volume, *self.attributes, o.disparity, extra, self.Q, self.world, self.origin, self.voxel,
                                self.trunc, **self._frame_kwargs(o))

    def __call__(self, left, right, motion=None, colors=None):
        given = left if colors is None else colors
        if not isinstance(given, torch.Tensor) or given.dim() != 4 or given.shape[:2] != (1, self.channels):
            raise ValueError(f"ColorStereoMapper: colors {tuple(getattr(given, 'shape', ()))}: [1,{self.channels},H,W]"
                             + (" (the left image: pass colors, or channels=3)" if colors is None else ""))
        # the disparity has the left image's size: a colour image of another size is refused here, before the tracker and the pose move
        if isinstance(left, torch.Tensor) and left.dim() == 4 and given.shape[2:] != left.shape[2:]:
            raise ValueError(f"ColorStereoMapper: colors {tuple(given.shape)} against the frames {tuple(left.shape)}: one size H x W")
        if isinstance(left, torch.Tensor) and given.device != left.device:
            raise ValueError(f"ColorStereoMapper: colors on {given.device}, the frames on {left.device}: one device")
        return self._frame(left, right, motion, given)

    def render_colors(self, T=None, size=None, near_disp=None, far_disp=None, step=0.5, max_steps=None, with_weight=False, Q_out=None):
        """color.volume_raycast with render()'s arguments and defaults: (disparity [1,1,H,W], colors [1,channels,H,W]), and
        hit_weight behind them with with_weight=True."""
        view = self._view("ColorStereoMapper.render_colors", T, size, near_disp, far_disp, Q_out)
        return _color.volume_raycast(*self.volume, *self.attributes, *view, step, max_steps, with_weight)

    def colored_mesh(self, min_weight=0.0, **kw):
        """(mesh(min_weight, **kw), its vertex colours [N,channels] fp32 by color.mesh_colors, in the same frame)."""
        self._need_frames("ColorStereoMapper.colored_mesh")
        m = self.mesh(min_weight, **kw)
        return m, _color.mesh_colors(m, *self.attributes, self.origin, self.voxel, kw.get("T"))
