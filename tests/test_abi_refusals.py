"""The refusal contract of every C entry point, without a device.

include/ecm_hip.h (and ecm_geometry.h / ecm_rectify.h, which inherit it): a bad argument returns a negative ECM_E* code --
ECM_EINVAL for a null pointer or a non-positive size, ECM_EUNSUP for a shape the kernels are not built for, ECM_ESCRATCH for a
short scratch buffer -- and a positive hipError_t means that a launch was attempted.  A refusal happens before any HIP call, so
with no device visible "refused" is a negative code and "reached the runtime" a positive one (hipErrorNoDevice), and the whole
contract can be held on the CPU: ROWS has one hand-written row per int-returning entry that takes a pointer, QUERIES one per
long long size query, and one child process (tests/abi_refusal_child.py, started with the GPUs hidden; it makes no ABI call if
it sees a device all the same) makes every call of the table.

A row's spec lists the entry's parameters in the header's order, `name:class` for pointers and `name=value` for scalars:
    x:p   required device pointer      x:o   optional device pointer (the header says it may be NULL)      x:s   the stream (NULL)
    x:x   a device pointer whose rule the row states itself, in inval / legal
    x:hi2 / x:hf3 / x:hf3@1   a HOST array the entry reads: int / float, its length, `@v` its fill (default 0)
    x:hP9                     a HOST array of 9 device pointers
    n=4      a size or count (int; `L4`: long long): 0 and -1 must return ECM_EINVAL;  `n=4%4`: and so must -4, minus its divisor
    n=?3     a choice (stride, dilation, kernel size, head count): it selects a kernel, so 0 and -1 must return ECM_EUNSUP
    n=-0     a value that may be 0: -1 must return ECM_EINVAL
    n=~1     a flag or free value: not probed;   x=f1.5   a float: not probed
    n=Q0     (long long) the result of the row's size query number 0 at the accepted sizes; one less must return ECM_ESCRATCH
unsup / inval / short / legal: further argument changes that must return ECM_EUNSUP / ECM_EINVAL / ECM_ESCRATCH / a positive
code; a value given as "ecm_lr_check_max_width+1" is that int query's result plus one, and a change of a Q parameter is an offset
to the query's result.  A size query must answer 0 (`refusal`, where its header comment documents another value for an ECM_EINVAL)
at every size vector that the call refuses, as far as the query's own arguments show the change; `blind` names the parameters, or
the single changes, for which a row states, with its source, why the query answers all the same.
codes: {(name, value): code} where the header gives a size probe another code than ECM_EINVAL, with the header line beside it."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import abi_refusal_child as child
from test_abi_types import HEADERS, declared, header_prototypes, lib_mod  # noqa: F401  (lib_mod builds the library if missing)

EINVAL, EUNSUP, ESCRATCH = -1, -2, -3
CODE = {EINVAL: "ECM_EINVAL", EUNSUP: "ECM_EUNSUP", ESCRATCH: "ECM_ESCRATCH"}
CTYPE = {"p": C.c_void_p, "i": C.c_int, "q": C.c_longlong, "f": C.c_float}


class Row:
    def __init__(self, name, spec, queries=(), unsup=(), inval=(), short=(), legal=(), codes=None, blind=(), refusal=0,
                 header="ecm_hip.h"):
        self.name, self.header, self.queries = name, header, list(queries)
        self.unsup, self.inval, self.short, self.codes = list(unsup), list(inval), list(short), dict(codes or {})
        self.legal, self.blind, self.refusal = list(legal), tuple(blind), refusal
        self.params = [_param(t) for t in spec.split()]
        self.types = [CTYPE[p["t"]] for p in self.params]
        names = [p["name"] for p in self.params]
        assert len(set(names)) == len(names), (name, names)

    def value(self, pname):
        return next(p["v"] for p in self.params if p["name"] == pname)


def _param(tok):
    if ":" in tok:
        name, cls = tok.split(":")
        if cls[0] == "h":
            fill = float(cls.split("@")[1]) if "@" in cls else 0
            kind, n = cls[1], int(cls[2:].split("@")[0])
            return {"name": name, "t": "p", "cls": "host", "host": kind, "n": n, "fill": int(fill) if kind == "i" else fill}
        return {"name": name, "t": "p", "cls": {"p": "req", "o": "opt", "s": "stream", "x": "own"}[cls]}
    name, val = tok.split("=")
    cls = {"?": "choice", "~": "flag", "-": "nonneg"}.get(val[0], "size")
    if cls != "size":
        val = val[1:]
    if val[0] == "f":
        return {"name": name, "t": "f", "cls": "float", "v": float(val[1:])}
    if val[0] == "Q":
        return {"name": name, "t": "q", "cls": "query", "q": int(val[1:])}
    t = "i"
    if val[0] == "L":
        t, val = "q", val[1:]
    div = None
    if "%" in val:
        val, div = val.split("%")
    return {"name": name, "t": t, "cls": cls, "v": int(val), "div": int(div) if div else None}


_NH = [{"nheads": 0}, {"nheads": 4}]                        # "nheads in 1..3" (ecm_hip.h, a8)
_HEADS = "nheads=?1 B=1 D=1 hw=1 stream:s"
_W4 = "W0:p W1:p W2:p W3:p"
_GN = "B=1 C=32%32 S=L1"
_GNQ = ("ecm_gn3d_scratch_bytes", "B C S")
_GNC = ("ecm_gn3d_cluster_bytes", "B")
_PREP = "mean3:hf3 std3:hf3@1"

ROWS = [
    # ---- a1: cost volume
    Row("ecm_costvol_concat_fwd", "L:p R:p cost:p B=1 C=1 h=1 w=1 D=1 stream:s"),
    Row("ecm_costvol_concat_bwd", "gcost:p gL:p gR:p B=1 C=1 h=1 w=1 D=1 stream:s"),
    # ---- a8: soft-argmin heads
    Row("ecm_softargmin_heads_fwd", "c0:p head_stride=-L8 disp:p " + _HEADS, unsup=_NH),
    Row("ecm_softargmin_heads_bwd", "c0:p head_stride=-L8 gdisp:p gc0:p " + _HEADS, unsup=_NH),
    Row("ecm_softargmin_heads_lse_fwd", "c0:p head_stride=-L8 disp:p lse:p " + _HEADS, unsup=_NH),
    Row("ecm_disparity_regression_fwd", "x:p out:p B=1 D=1 hw=1 stream:s"),
    # ---- a9: nine-neighbour aggregation
    Row("ecm_aggregate9_fwd", "d:p w9:p out:p nheads=?1 B=1 h=1 w=1 s=4 stream:s", unsup=_NH),
    Row("ecm_aggregate9_bwd", "d:p w9:p gout:p gd:p gw9:p nheads=?1 B=1 h=1 w=1 s=4 stream:s", unsup=_NH),
    Row("ecm_aggregate9_stats_fwd", "c0:p head_stride=-L8 lse:p w9:p stats:p nheads=?1 B=1 D=1 h=1 w=1 s=4 stream:s", unsup=_NH),
    Row("ecm_aggregate9_mode_fwd",
        "c0:p head_stride=-L8 lse:p w9:p modal:p nheads=?1 B=1 D=1 h=1 w=1 s=4 radius=-0 stream:s",
        unsup=_NH + [{"B": 65536}], inval=[{"radius": 2}]),                # "a multiple of s (else ECM_EINVAL)", "B > 65535"
    # ---- a3 / a4: context-mapping weights
    Row("ecm_weights9_fwd", f"lr:p hr:p {_W4} w9:p scratch:p scratch_bytes=Q0 B=1 h=1 w=1 s=4 stream:s",
        queries=[("ecm_weights9_scratch_bytes", "B h w")]),
    Row("ecm_weights9_bwd",
        f"lr:p hr:p {_W4} w9:p gw9:p glr:p ghr:p gW:p scratch:p scratch_bytes=Q0 B=1 h=1 w=1 s=4%4 stream:s",
        queries=[("ecm_weights9_bwd_scratch_bytes", "B h w s")], unsup=[{"s": 6}]),
    Row("ecm_context_weights_fwd", f"lr:p hr:p {_W4} out:p scratch:p scratch_bytes=Q0 B=1 h=1 w=1 s=2%2 variant=~1 stream:s",
        queries=[("ecm_weights9_scratch_bytes", "B h w")],
        unsup=[{"s": 3}, {"variant": 3}, {"variant": -1}, {"variant": 0}]),   # "Any even scale s"; variant 0 is built for s = 4
    Row("ecm_context_weights_bwd",
        f"lr:p hr:p {_W4} out_saved:p gout:p glr:p ghr:p gW:p scratch:p scratch_bytes=Q0 B=1 h=1 w=1 s=4%4 variant=~0 stream:s",
        queries=[("ecm_context_weights_bwd_scratch_bytes", "B h w s variant")], unsup=[{"s": 6}, {"variant": 3}, {"variant": -1}]),
    # ---- a10: volume mapping
    Row("ecm_volume_mapping_fwd", "c0:p head_stride=-L8 m5:p mt3:p disp:p nheads=?1 B=1 Dl=1 h=1 w=1 s=2 stream:s", unsup=_NH),
    Row("ecm_volume_mapping_stats_fwd",
        "c0:p head_stride=-L8 m5:p mt3:p disp:p stats:p nheads=?1 B=1 Dl=1 h=1 w=1 s=2 stream:s", unsup=_NH),
    Row("ecm_volume_mapping_mode_fwd",
        "c0:p head_stride=-L8 m5:p mt3:p modal:p nheads=?1 B=1 Dl=1 h=1 w=1 s=2 radius=-0 stream:s", unsup=_NH),
    Row("ecm_volume_mapping_bwd",
        "c0:p head_stride=-L8 m5:p mt3:p gdisp:p gc0:p gm5:p gmt3:p scratch:p scratch_bytes=Q0 nheads=?1 B=1 Dl=1 h=1 w=1 s=2 stream:s",
        queries=[("ecm_volume_mapping_bwd_scratch_bytes", "nheads B Dl h w s")],
        unsup=_NH + [{"s": 3}, {"s": 128}]),                               # "s must be a power of two <= 64"
    # ---- a11: trilinear head
    Row("ecm_trilinear_softargmin_fwd", "c0:p head_stride=-L8 disp:p nheads=?1 B=1 Dl=1 h=1 w=1 Do=1 H=1 W=1 stream:s", unsup=_NH),
    Row("ecm_trilinear_softargmin_stats_fwd",
        "c0:p head_stride=-L8 disp:p stats:p nheads=?1 B=1 Dl=1 h=1 w=1 Do=1 H=1 W=1 stream:s", unsup=_NH),
    Row("ecm_trilinear_softargmin_mode_fwd",
        "c0:p head_stride=-L8 modal:p nheads=?1 B=1 Dl=1 h=1 w=1 Do=1 H=1 W=1 radius=-0 stream:s", unsup=_NH),
    Row("ecm_trilinear_softargmin_bwd",
        "c0:p head_stride=-L8 gdisp:p gc0:p scratch:p scratch_bytes=Q0 nheads=?1 B=1 Dl=1 h=1 w=1 Do=1 H=1 W=1 stream:s",
        queries=[("ecm_trilinear_softargmin_bwd_scratch_bytes", "nheads B Dl h w H W")], unsup=_NH),
    # ---- a5-a7: 3-D aggregation
    Row("ecm_conv3d_pack_weight", "w:p packed:p Co=1 Ci=4 flip_transpose=~0 stream:s"),
    Row("ecm_conv3d_k3_fwd", "x:p wpacked:p y:p B=1 Ci=4%4 Co=1 D=1 H=1 W=1 stride=?1 stream:s",
        unsup=[{"Ci": 5}, {"Co": 65}, {"stride": 3}]),                     # "Ci % 4 == 0; 1 <= Co <= 64", "st in {1,2}"
    Row("ecm_conv_wino_pack_weight", "w:p packed:p Co=1 Ci=1 kd=?3 flip_transpose=~0 stream:s", unsup=[{"kd": 2}]),
    Row("ecm_conv_wino_pack_weight2", "w:p packed:p Co=1 Ci=1 kd=?3 stream:s", unsup=[{"kd": 2}]),
    Row("ecm_conv_wino_fwd", "x:p upacked:p y:p B=1 Ci=1 Co=1 D=1 H=1 W=2 kd=?3 stream:s", unsup=[{"kd": 2}]),
    Row("ecm_conv_wino_fwd_add", "x:p upacked:p addend:p y:p B=1 Ci=1 Co=1 D=1 H=1 W=2 kd=?3 stream:s", unsup=[{"kd": 2}]),
    Row("ecm_conv_wino_wgrad", "x:p gy:p gw:p scratch:p scratch_bytes=Q0 B=1 Ci=4 Co=4 D=1 H=2 W=2 kd=?3 stream:s",
        queries=[("ecm_conv_wino_wgrad_scratch_bytes", "B Ci Co D H W kd")], unsup=[{"kd": 2}]),
    Row("ecm_sum_n", "a:p b:p c:x d:o out:p n=L4 stream:s", inval=[{"c": None}], legal=[{"c": None, "d": None}]),   # d only with c
    Row("ecm_zero_insert2d", "small:p out:p planes=L1 H=2 W=2 Hs=1 Ws=1 stream:s"),
    Row("ecm_conv3d_c1_fwd", "x:p w:p y:p B=1 Ci=4 D=1 H=1 W=1 stream:s", unsup=[{"Ci": 33}]),     # "Conv3d(Ci<=32 -> 1)"
    Row("ecm_conv3d_c1_dgrad", "gy:p w:p gx:p B=1 Ci=1 D=1 H=1 W=1 stream:s"),
    Row("ecm_conv3d_c1_wgrad", "x:p gy:p gw:p scratch:p scratch_bytes=Q0 B=1 Ci=4 D=1 H=1 W=1 stream:s",
        queries=[("ecm_conv3d_c1_wgrad_scratch_bytes", "B Ci D H W")]),
    Row("ecm_conv3d_c1_gn_fwd", "x:p mean_rstd:p gamma:p beta:p w:p y:p B=1 Ci=32 D=1 H=1 W=1 stream:s",
        unsup=[{"Ci": 16}, {"Ci": 64}]),                                   # "Ci must be 32"
    Row("ecm_conv3d_c1_gn_wgrad",
        "x:p mean_rstd:p gamma:p beta:p gy:p gw:p scratch:p scratch_bytes=Q0 B=1 Ci=32 D=1 H=1 W=1 stream:s",
        queries=[("ecm_conv3d_c1_wgrad_scratch_bytes", "B 32 D H W")], unsup=[{"Ci": 16}, {"Ci": 64}]),   # ecm_conv3d_c1_wgrad's query
    Row("ecm_deconv3d_pack_weight", "w:p packed:p Ci=4 Co=1 stream:s"),
    Row("ecm_deconv3d_k3s2_fwd", "x:p wpacked:p y:p B=1 Ci=4%4 Co=1 D=1 H=1 W=1 Do=2 Ho=2 Wo=2 stream:s",
        unsup=[{"Ci": 5}, {"Co": 65}, {"Do": 3}, {"Ho": 3}, {"Wo": 3}]),   # "Do = 2D (or 2D-1 ...)"
    Row("ecm_conv3d_k3_wgrad", "x:p gy:p gw:p scratch:p scratch_bytes=Q0 B=1 Ci=4 Co=4 D=1 H=1 W=1 stride=?1 stream:s",
        queries=[("ecm_conv3d_wgrad_scratch_bytes", "B Ci Co D H W stride")], unsup=[{"stride": 3}]),
    # ---- 2-D convolution family
    Row("ecm_conv2d_pack_weight_ex", "w:p packed:p Co=1 Ci=4 kh=3 kw=3 flip_transpose=~0 stream:s"),       # any [Co,Ci,kh,kw]: sizes
    Row("ecm_conv2d_fwd_ex",
        "x:p wpacked:p y:p B=1 Ci=4 Co=1 H=1 W=1 kh=?3 kw=?3 stride=?1 dil=?1 pad_top=~1 pad_left=~1 Ho=1 Wo=1 stream:s",
        unsup=[{"stride": 3}, {"dil": 3}, {"kh": 5}, {"kw": 7}]),          # "(kh,kw,stride,dil) in {...}"
    Row("ecm_conv2d_wgrad_ex",
        "x:p gy:p gw:p scratch:p scratch_bytes=Q0 B=1 Ci=4 Co=1 H=1 W=1 kh=?3 kw=?3 stride=?1 dil=?1 pad_top=~1 pad_left=~1 "
        "Ho=1 Wo=1 stream:s",
        queries=[("ecm_conv2d_wgrad_ex_scratch_bytes", "B Ci Co Ho Wo kh kw stride")],
        # outside the (kh, kw, stride) table the query still answers (csrc/conv3d_wgrad.hip, wg2_query_plan) and a short scratch
        # is reported first (test_wgrad_plan_cpu.py::test_scratch_is_refused_before_the_gpu): with room, "no such kernel"
        blind=("kh", "kw", "stride"),
        unsup=[{"stride": 3, "scratch_bytes": 1 << 30}, {"dil": 3}, {"kh": 5, "scratch_bytes": 1 << 30},
               {"kw": 7, "scratch_bytes": 1 << 30}], short=[{"kh": 5}]),
    Row("ecm_deconv2d_pack_weight", "w:p packed:p Ci=4 Co=1 stream:s"),
    Row("ecm_deconv2d_k3s2_fwd", "x:p wpacked:p y:p B=1 Ci=4%4 Co=1 H=1 W=1 Ho=2 Wo=2 stream:s",
        unsup=[{"Ci": 5}, {"Co": 65}, {"Ho": 3}, {"Wo": 3}]),              # "Co <= 64, Ci % 4 == 0", "Ho in {2H-1, 2H}"
    # ---- cmf decoder
    Row("ecm_deconv2d_k3s2_bias_fwd", "x:p wpacked:p bias:p y:p B=1 Ci=4%4 Co=1 H=1 W=1 Ho=2 Wo=2 stream:s",
        unsup=[{"Ci": 5}, {"Co": 65}, {"Ho": 3}, {"Wo": 3}]),
    Row("ecm_channel_sum", "x:p out:p scratch:p scratch_bytes=Q0 B=1 C=1 HW=L1 stream:s",
        queries=[("ecm_channel_sum_scratch_bytes", "B C HW")]),
    Row("ecm_conv2d_c1_fwd", "x:p w:p bias:p y:p B=1 Ci=1 H=1 W=1 stream:s"),
    Row("ecm_conv2d_c1_dgrad", "gy:p y:p w:p gx:p B=1 Ci=1 H=1 W=1 stream:s"),
    Row("ecm_conv2d_c1_wgrad", "x:p gy:p y:p gw:p gb:p scratch:p scratch_bytes=Q0 B=1 Ci=1 H=1 W=1 stream:s",
        queries=[("ecm_conv2d_c1_wgrad_scratch_bytes", "B Ci H W")]),
    # ---- GroupNorm
    Row("ecm_gn3d_fwd", f"x:p gamma:p beta:p skip:o y:p mean_rstd:p scratch:p scratch_bytes=Q0 {_GN} relu=~1 eps=f1e-5 stream:s",
        queries=[_GNQ], unsup=[{"C": 33}]),
    Row("ecm_gn3d_stats", f"x:p mean_rstd:p scratch:p scratch_bytes=Q0 {_GN} eps=f1e-5 stream:s", queries=[_GNQ], unsup=[{"C": 33}]),
    Row("ecm_gn3d_stats_bf16", f"x:p mean_rstd:p scratch:p scratch_bytes=Q0 {_GN} eps=f1e-5 stream:s", queries=[_GNQ],
        unsup=[{"C": 33}]),
    Row("ecm_gn3d_apply", f"x:p mean_rstd:p gamma:p beta:p skip:o y:p {_GN} relu=~1 stream:s", unsup=[{"C": 33}]),
    Row("ecm_gn3d_apply_bf16", f"x:p mean_rstd:p gamma:p beta:p skip:o y:p {_GN} relu=~1 stream:s", unsup=[{"C": 33}]),
    Row("ecm_gn3d_apply_f32_bf16", f"x:p mean_rstd:p gamma:p beta:p skip:o y:p {_GN} relu=~1 stream:s", unsup=[{"C": 33}]),
    Row("ecm_gn3d_apply_bf16_f32", f"x:p mean_rstd:p gamma:p beta:p skip:o y32:p y16:o {_GN} relu=~1 stream:s", unsup=[{"C": 33}]),
    Row("ecm_gn3d_bwd",
        f"x:p mean_rstd:p gamma:p beta:o y:o gy:p gx:p gskip:o ggamma:p gbeta:p scratch:p scratch_bytes=Q0 {_GN} relu=~1 stream:s",
        queries=[_GNQ], unsup=[{"C": 33}]),
    Row("ecm_costvol_class_weights_fwd", "w:p wP:p wQ:p Co=1 C=1 stream:s"),
    Row("ecm_costvol_class_weights_bwd", "gwP:p gwQ:p gw:p Co=1 C=1 stream:s"),
    Row("ecm_gn3d_cluster_preset", "cluster:p cluster_bytes=L64 stream:s"),         # fills what it is given: any positive size
    Row("ecm_gn3d_fwd_p",
        f"x:p gamma:p beta:p skip:o y:p mean_rstd:p scratch:p scratch_bytes=Q0 cluster:p cluster_bytes=Q1 {_GN} relu=~1 eps=f1e-5 "
        "stream:s", queries=[_GNQ, _GNC], unsup=[{"C": 33}]),
    Row("ecm_gn3d_bwd_p",
        f"x:p mean_rstd:p gamma:p beta:o y:o gy:p gx:p gskip:o ggamma:p gbeta:p scratch:p scratch_bytes=Q0 cluster:p "
        f"cluster_bytes=Q1 {_GN} relu=~1 stream:s", queries=[_GNQ, _GNC], unsup=[{"C": 33}]),
    Row("ecm_costvol_conv_assemble_fwd", "P:p Qp:p y:p B=1 Co=1 D=2 h=1 w=1 stream:s", unsup=[{"D": 1}]),      # "D >= 2 (D = 1: ECM_EUNSUP"
    Row("ecm_costvol_conv_assemble_bwd", "gy:p gP:p gQp:p B=1 Co=1 D=2 h=1 w=1 stream:s", unsup=[{"D": 1}]),
    # ---- harness input side
    Row("ecm_frame_prep",
        f"frames:p left:p right:p disp:p image:o B=1 H=2 W=2 crop_y0:hi1 crop_x0:hi1 th=1 tw=1 split=~1 tail=~0 {_PREP} stream:s",
        inval=[{"th": 3}, {"tw": 3}]),                                     # a window that leaves the frame: the arguments disagree
    Row("ecm_frame_prep_kitti_eval", f"frames:p left:p right:p disp:p image:o B=1 H=2 W=2 th=2 tw=2 {_PREP} stream:s",
        inval=[{"th": 5}, {"tw": 5}, {"th": 1}]),                          # "Needs th-H <= H, tw-W <= W"
    Row("ecm_frame_prep_packed",
        "rgb6:p disp_in:p disp_is_half=~0 left:p right:p disp:p image:o B=1 H=2 W=2 crop_y0:hi1 crop_x0:hi1 th=1 tw=1 split=~1 "
        f"tail=~0 {_PREP} mode=~0 stream:s", inval=[{"th": 3}, {"tw": 3}], unsup=[{"mode": 2}, {"mode": -1}]),
    # ---- evaluation
    Row("ecm_eval_epe",
        "pred:p gt:p out6:p scratch:p scratch_bytes=Q0 B=1 Hp=1 Wp=1 Hg=1 Wg=1 crop_h=1 crop_w=1 maxdisp=f192 stream:s",
        queries=[("ecm_eval_epe_scratch_bytes", "B*crop_h*crop_w")], inval=[{"crop_h": 2}, {"crop_w": 2}],
        blind=("crop_h=2", "crop_w=2")),                                   # a crop beyond the maps: the query sees only n
    Row("ecm_eval_kitti", "pred:p gt:p out8:p per_sample:o scratch:p scratch_bytes=Q0 B=1 H=1 W=1 maxdisp=f192 stream:s",
        queries=[("ecm_eval_kitti_scratch_bytes", "B H W")], unsup=[{"B": 65536}, {"H": 65536, "W": 32768}]),                # "B > 65535: ECM_EUNSUP"
    Row("ecm_eval_sparsify",
        "pred:p gt:p measures:hP9 table:p count:p scratch:p scratch_bytes=Q0 B=1 H=1 W=1 K=1 steps=1 maxdisp=f192 stream:s",
        queries=[("ecm_eval_sparsify_scratch_bytes", "B H W K steps")],
        unsup=[{"B": 65536}, {"H": 65536, "W": 32768}, {"K": "ecm_eval_sparsify_max_measures+1"}, {"steps": "ecm_eval_sparsify_max_steps+1"}]),
    Row("ecm_disp_to_u16", "pred:p out:p B=1 Hp=1 Wp=1 h:hi1@1 w:hi1@1 Ho=1 Wo=1 scale=f256 stream:s"),
    # ---- post-processing
    Row("ecm_lr_check_fwd", "dl:p dr:p check:p src:o B=1 H=1 W=1 threshold=f1 rel=f0 mirrored=~0 stream:s",
        unsup=[{"W": "ecm_lr_check_max_width+1"}, {"B": 65536, "H": 32768}]),                        # "B * H >= 2^31"
    Row("ecm_disp_median_fwd", "d:p valid:o out:p B=1 H=1 W=1 radius=1 stream:s", inval=[{"radius": 4}], unsup=[{"B": 128, "H": 4096, "W": 4096}]),    # "a radius out of range"
    Row("ecm_disp_bilateral_fwd", "d:p valid:o guide:p out:p B=1 C=1 H=1 W=1 radius=1 sigma_space=f1 sigma_color=f1 stream:s",
        inval=[{"radius": 9}, {"C": 5}], unsup=[{"B": 128, "H": 4096, "W": 4096}]),                                  # "C outside 1..4"
    Row("ecm_disp_speckle_fwd", "d:p valid:o out:p segments:p B=1 H=1 W=1 max_size=-0 max_diff=f1 stream:s", unsup=[{"B": 128, "H": 4096, "W": 4096}]),        # "B * H * W >= 2^31"
    Row("ecm_disp_wls_fwd", "d:p conf:o guide:p out:p scratch:p B=1 C=1 H=1 W=1 lam=f1 sigma_color=f1 iterations=1 stream:s",
        queries=[("ecm_disp_wls_scratch_bytes", "B H W")], inval=[{"C": 5}, {"iterations": 9}], unsup=[{"B": 128, "H": 4096, "W": 4096}]),   # "iterations outside 1..8"
    Row("ecm_disp_splat_fwd", "dl:p right:p src:o B=1 H=1 W=1 stream:s", unsup=[{"W": "ecm_disp_splat_max_width+1"}, {"B": 65536, "H": 32768}]),
    # ---- loss
    Row("ecm_stereo_loss_fwd",
        "p1:p p2:p p3:p gt:p out8:p scratch:p scratch_bytes=Q0 n=L1 maxdisp=f192 w1=f0.5 w2=f0.7 w3=f1 stream:s",
        queries=[("ecm_stereo_loss_scratch_bytes", "n")]),
    Row("ecm_stereo_loss_bwd",
        "p1:p p2:p p3:p gt:p out8:p gloss:p g1:p g2:p g3:p n=L1 maxdisp=f192 w1=f0.5 w2=f0.7 w3=f1 stream:s"),
    # ---- bf16 inference, 3-D
    Row("ecm_conv3d_bf16_pack_weight", "w:p packed:p Ci=32%8 Co=32 transposed=~0 stream:s", unsup=[{"Ci": 12}]),
    Row("ecm_conv3d_k3_bf16_fwd", "x:p wpacked:p y:p B=1 Ci=32 Co=32 D=1 H=1 W=1 stride=?1 stream:s",
        unsup=[{"Ci": 16}, {"Co": 16}, {"Ci": 128}, {"stride": 3}]),                     # "Ci, Co in {32, 64}"
    Row("ecm_deconv3d_k3s2_bf16_fwd", "x:p wpacked:p y:p B=1 Ci=32 Co=32 D=1 H=1 W=1 stream:s",
        unsup=[{"Ci": 16}, {"Co": 16}, {"Co": 128}]),
    Row("ecm_conv3d_c1_gn_fwd_bf16", "x:p mean_rstd:p gamma:p beta:p w:p y:p B=1 Ci=32 D=1 H=1 W=1 stream:s",
        unsup=[{"Ci": 16}, {"Ci": 64}]),
    # ---- bf16 inference, encoder and decoder
    Row("ecm_conv2d_bf16_pack_weight", "w:p packed:p Ci=16%16 Co=32 k=?3 stream:s", unsup=[{"Ci": 8}, {"k": 2}]),
    Row("ecm_conv2d_bf16_fwd", "x:p wpacked:p y:p B=1 Ci=16%16 Co=32%32 H=1 W=1 k=?3 stride=?1 dil=?1 out_f32=~0 stream:s",
        unsup=[{"Ci": 8}, {"Co": 16}, {"stride": 3}, {"dil": 3}, {"k": 2}]),             # "Ci % 16 == 0, Co % 32 == 0"
    Row("ecm_deconv2d_bf16_pack_weight", "w:p packed:p Ci=16%16 Co=32 stream:s", unsup=[{"Ci": 8}, {"Co": 16}]),
    Row("ecm_deconv2d_k3s2_bias_bf16_fwd", "x:p wpacked:p bias:p y:p B=1 Ci=16%16 Co=32 H=1 W=1 stream:s",
        unsup=[{"Ci": 8}, {"Co": 16}, {"Co": 128}]),                       # "Ci % 16 == 0, Co in {32, 64}"
    Row("ecm_conv2d_c1_bf16_fwd", "x:p w:p bias:p y:p B=1 Ci=16%16 H=1 W=1 stream:s", unsup=[{"Ci": 8}, {"Ci": 1040}]),
    # ---- split-bf16
    Row("ecm_conv3d_split_pack_weight", "w:p packed:p Ci=32%8 Co=32 transposed=~0 stream:s", unsup=[{"Ci": 12}]),
    Row("ecm_conv3d_k3s2_split_fwd", "x:p wpacked:p y:p B=1 Ci=32 Co=32 D=1 H=1 W=1 stream:s",
        unsup=[{"Ci": 16}, {"Co": 16}, {"Ci": 128}]),                      # "Ci, Co in {32, 64} ... anything else ECM_EUNSUP"
    Row("ecm_deconv3d_k3s2_split_fwd", "x:p wpacked:p y:p B=1 Ci=32 Co=32 D=1 H=1 W=1 Do=2 Ho=2 Wo=2 stream:s",
        unsup=[{"Ci": 16}, {"Co": 16}, {"Co": 128}, {"Do": 3}, {"Ho": 3}, {"Wo": 3}]),
    # ---- ecm_geometry.h
    Row("ecmg_reproject_fwd", "disp:p valid:o Q:p q_per_image=~0 xyz:p mask:o B=1 H=1 W=1 min_disp=f0 max_disp=f100 stream:s",
        unsup=[{"B": 128, "H": 4096, "W": 4096}], header="ecm_geometry.h"),
    Row("ecmg_point_cloud_fwd",
        "disp:p valid:o Q:p q_per_image=~0 attrs:o C=-0 points:p offsets:p xyz:o mask:o scratch:p scratch_bytes=Q0 B=1 H=1 W=1 "
        "min_disp=f0 max_disp=f100 stream:s", queries=[("ecmg_point_cloud_scratch_bytes", "B H W")],
        inval=[{"C": 5}, {"C": 1, "attrs": None}], unsup=[{"B": 128, "H": 4096, "W": 4096}], header="ecm_geometry.h"),                       # "C outside 0..4, attrs null with C > 0"
    # ---- ecm_rectify.h
    Row("ecmr_rectify_map_fwd", "params:p map:p Ho=1 Wo=1 stream:s", unsup=[{"Ho": 262141}], header="ecm_rectify.h"),
    Row("ecmr_remap_pair_fwd",
        "left_raw:p right_raw:p src_is_u8=~1 map_left:p map_right:p map_per_image=~0 left:p right:p image:o mask_left:o "
        f"mask_right:o B=1 H=2 W=2 Ho=1 Wo=1 {_PREP} border=f0 stream:s",
        unsup=[{"B": 32768}, {"H": (1 << 24) + 1}, {"W": (1 << 24) + 1}, {"Ho": 1048561}], header="ecm_rectify.h"),
]
ROW = {r.name: r for r in ROWS}

# int entries with a pointer parameter that have no row: name -> the reason
ACCOUNTED_FOR = {}

# every long long size query: accepted arguments (> 0), and 0 for a zero or negative size or choice, never a negative value
QUERIES = [
    Row("ecm_weights9_scratch_bytes", "B=1 h=1 w=1"),
    Row("ecm_weights9_bwd_scratch_bytes", "B=1 h=1 w=1 s=4"),
    Row("ecm_context_weights_bwd_scratch_bytes", "B=1 h=1 w=1 s=4 variant=~0"),
    Row("ecm_volume_mapping_bwd_scratch_bytes", "nheads=?1 B=1 Dl=1 h=1 w=1 s=2"),
    Row("ecm_trilinear_softargmin_bwd_scratch_bytes", "nheads=?1 B=1 Dl=1 h=1 w=1 H=1 W=1"),
    Row("ecm_conv3d_packed_floats", "Ci=4 Co=1"),
    Row("ecm_conv_wino_packed_floats", "Ci=1 Co=1 kd=?3"),
    Row("ecm_conv_wino_wgrad_scratch_bytes", "B=1 Ci=4 Co=4 D=1 H=2 W=2 kd=?3"),
    Row("ecm_conv3d_c1_wgrad_scratch_bytes", "B=1 Ci=4 D=1 H=1 W=1"),
    Row("ecm_conv3d_wgrad_scratch_bytes", "B=1 Ci=4 Co=4 D=1 H=1 W=1 stride=?1"),
    Row("ecm_conv2d_packed_floats_ex", "Ci=4 Co=1 kh=3 kw=3"),
    Row("ecm_conv2d_wgrad_ex_scratch_bytes", "B=1 Ci=4 Co=1 Ho=1 Wo=1 kh=?3 kw=?3 stride=~1"),    # any stride but 1 counts as 2
    Row("ecm_channel_sum_scratch_bytes", "B=1 C=1 HW=L1"),
    Row("ecm_conv2d_c1_wgrad_scratch_bytes", "B=1 Ci=1 H=1 W=1"),
    Row("ecm_gn3d_scratch_bytes", "B=1 C=32 S=L1"),
    Row("ecm_gn3d_cluster_bytes", "B=1"),
    Row("ecm_eval_epe_scratch_bytes", "n=L1"),
    Row("ecm_eval_kitti_scratch_bytes", "B=1 H=1 W=1"),
    Row("ecm_eval_sparsify_scratch_bytes", "B=1 H=1 W=1 K=1 steps=1"),
    Row("ecm_disp_wls_scratch_bytes", "B=1 H=1 W=1", refusal=EINVAL),  # ecm_hip.h, ABI 13: "ECM_EINVAL ... (the size query: B, H or W < 1)"
    Row("ecm_stereo_loss_scratch_bytes", "n=L1"),
    Row("ecm_conv3d_bf16_packed_elems", "Ci=32 Co=32"),
    Row("ecm_conv2d_bf16_packed_elems", "Ci=16 Co=32 k=?3"),
    Row("ecm_deconv2d_bf16_packed_elems", "Ci=16 Co=32"),
    Row("ecm_conv3d_split_packed_elems", "Ci=32 Co=32"),
    Row("ecmg_point_cloud_scratch_bytes", "B=1 H=1 W=1", header="ecm_geometry.h"),
]
QUERY = {r.name: r for r in QUERIES}
INT_CONSTS = ("ecm_lr_check_max_width", "ecm_disp_splat_max_width", "ecm_eval_sparsify_max_measures", "ecm_eval_sparsify_max_steps")


# ---- from a row to calls, and from return codes to findings -------------------------------------------------------------------

def _fmt(change):
    return ",".join(f"{k}={'NULL' if v is None else v}" for k, v in change.items()) or "accepted"


def probes(row):
    """[(label, change, want)] of a row: change = {name: value | None}; want = "pos", "neg" or an exact code."""
    out = [("accepted", {}, "pos")]
    for p in row.params:
        n, cls = p["name"], p["cls"]
        if cls in ("req", "host"):
            out.append((f"{n}=NULL", {n: None}, EINVAL))
        elif cls == "opt":
            out.append((f"{n}=NULL", {n: None}, "pos"))
        elif cls in ("size", "choice"):
            for v in [0, -1] + ([-p["div"]] if p["div"] else []):
                want = row.codes.get((n, v), EINVAL if cls == "size" else EUNSUP)
                out.append((f"{n}={v}", {n: v}, want))
        elif cls == "nonneg":
            out.append((f"{n}=-1", {n: -1}, row.codes.get((n, -1), EINVAL)))
        elif cls == "query":
            out.append((f"{n}=query-1", {n: -1}, ESCRATCH))               # for a query parameter the change is the offset
    for changes, want in ((row.unsup, EUNSUP), (row.inval, EINVAL), (row.short, ESCRATCH), (row.legal, "pos")):
        out += [(_fmt(c), dict(c), want) for c in changes]
    last = {label: i for i, (label, _, _) in enumerate(out)}               # a value the row names itself replaces the generic probe
    return [p for i, p in enumerate(out) if last[p[0]] == i]


def _query_args(row, qi, change):
    """The arguments of size query qi at the row's values under `change`, or None where the change does not touch them."""
    qname, exprs = row.queries[qi]
    env = {p["name"]: change.get(p["name"], p["v"]) for p in row.params if "v" in p}
    if change and not any(re.search(rf"\b{re.escape(k)}\b", exprs) for k in change):
        return None
    if any(isinstance(env.get(k), str) for k in env):
        return None                                                        # a value that is itself a query's result
    return [int(eval(e, {"__builtins__": {}}, env)) for e in exprs.split()]


def _scalar(t, v):
    if isinstance(v, str):                                                 # "ecm_x_max+1"
        name, add = v.split("+")
        return {"t": t, "ref": f"const|{name}", "add": int(add)}
    return {"t": t, "v": v}


def calls_of(row, types_of):
    """The child's calls for one row: its size queries at the accepted sizes, every probe, and the query at every refused size
    vector that the query can see."""
    calls = []
    for qi, (qname, _) in enumerate(row.queries):
        qt = types_of(qname)
        calls.append({"id": f"{row.name}|query{qi}", "fn": qname, "res": "q",
                      "args": [{"t": "q" if t is C.c_longlong else "i", "v": v} for t, v in zip(qt, _query_args(row, qi, {}))]})
    for label, change, want in probes(row):
        args = []
        for i, p in enumerate(row.params):
            n, cls = p["name"], p["cls"]
            if cls == "query":
                args.append({"t": "q", "ref": f"{row.name}|query{p['q']}", "add": change.get(n, 0)})
            elif cls == "stream":
                args.append({"t": "p", "v": None})
            elif p["t"] == "p":
                if n in change:
                    args.append({"t": "p", "v": None})
                elif cls == "host":
                    args.append({"t": "p", "ptrs": p["n"]} if p["host"] == "P" else {"t": "p", "host": p["host"], "vals": [p["fill"]] * p["n"]})
                else:
                    args.append({"t": "p", "v": "dev", "off": 256 * i})
            else:
                args.append(_scalar(p["t"], change.get(n, p["v"])))
        calls.append({"id": f"{row.name}|{label}", "fn": row.name, "res": "i", "args": args})
        seen_by_query = label not in row.blind and not any(k in row.blind for k in change)
        if want != "pos" and label != "accepted" and seen_by_query:
            for qi, (qname, _) in enumerate(row.queries):
                qa = _query_args(row, qi, change)
                if qa is not None:
                    qt = types_of(qname)
                    calls.append({"id": f"{row.name}|query{qi}@{label}", "fn": qname, "res": "q",
                                  "args": [{"t": "q" if t is C.c_longlong else "i", "v": v} for t, v in zip(qt, qa)]})
    return calls


def _name(rc):
    return CODE.get(rc, str(rc))


def classify(row, got):
    """Every breach of the contract in the return codes `got` {call id: value} of calls_of(row): (entry, argument, got, wanted)."""
    bad = []
    rc = got[f"{row.name}|accepted"]
    if rc <= 0:
        return [(row.name, "accepted call", _name(rc), "a positive hipError_t: the call must reach the runtime")]
    for qi in range(len(row.queries)):
        q = got[f"{row.name}|query{qi}"]
        if q <= 0:
            bad.append((row.name, f"{row.queries[qi][0]} at the accepted sizes", str(q), "> 0"))
    for label, change, want in probes(row)[1:]:
        rc = got[f"{row.name}|{label}"]
        ok = rc > 0 if want == "pos" else rc < 0 if want == "neg" else rc == want
        if not ok:
            wanted = {"pos": "a positive hipError_t (the value is legal)", "neg": "a negative ECM_E* code"}.get(want) or _name(want)
            bad.append((row.name, label, _name(rc), wanted))
        for qi in range(len(row.queries)):
            q = got.get(f"{row.name}|query{qi}@{label}")
            none = getattr(QUERY.get(row.queries[qi][0]), "refusal", 0) if want == EINVAL else 0
            if q is not None and q != none:
                bad.append((row.name, f"{row.queries[qi][0]} at {label}", str(q), f"{none}: the call refuses these sizes"))
    return bad


def query_calls(row):
    calls = []
    for label, change, _ in probes(row):
        args = [_scalar(p["t"], change.get(p["name"], p["v"])) for p in row.params]
        calls.append({"id": f"{row.name}|{label}", "fn": row.name, "res": "q", "args": args})
    return calls


def classify_query(row, got):
    bad = []
    for label, change, _ in probes(row):
        v = got[f"{row.name}|{label}"]
        if label == "accepted" and v <= 0:
            bad.append((row.name, "accepted sizes", str(v), "> 0"))
        elif label != "accepted" and v != row.refusal:
            bad.append((row.name, label, str(v), str(row.refusal)))
    return bad


def _report(bad):
    return "\n".join(f"{e}: {a}: returned {g}, the contract wants {w}" for e, a, g, w in bad)


# ---- the child ---------------------------------------------------------------------------------------------------------------

HIDE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1", "GPU_DEVICE_ORDINAL": "-1"}


@pytest.fixture(scope="module")
def results(lib_mod):
    """{call id: return value} of the whole table from ONE fresh child that sees no device; the module skips if it sees one."""
    parsed = {}
    for h in HEADERS:
        parsed.update(header_prototypes(h))
    calls = [{"id": f"const|{n}", "fn": n, "res": "i", "args": []} for n in INT_CONSTS]
    for row in ROWS:
        calls += calls_of(row, lambda q: parsed[q][1])
    for row in QUERIES:
        calls += query_calls(row)
    assert len({c["id"] for c in calls}) == len(calls)
    env = dict(os.environ)
    env.update(HIDE)
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__)], input=json.dumps({"lib": lib_mod.LIB_PATH, "calls": calls}),
                       capture_output=True, text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    seen = next((ln.split()[1] for ln in lines if ln.startswith("DEVICES ")), None)
    assert seen is not None, f"the child did not report a device count (exit {r.returncode}): {r.stderr[-2000:]}"
    assert seen.isdigit(), f"the child could not ask the HIP runtime for its device count: {seen}"
    if seen != "0":
        pytest.skip(f"the child sees {seen} device(s) although {sorted(HIDE)} hide them: no ABI call was made")
    got = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("R ")}
    if "DONE" not in lines:
        nxt = next((c["id"] for c in calls if c["id"] not in got), None)
        pytest.fail(f"the child ended with status {r.returncode} in call {nxt}: {r.stderr[-2000:]}")
    return got


# ---- the census --------------------------------------------------------------------------------------------------------------

def _entries(header):
    """(entries, queries): the int entries with a pointer parameter, and the long long functions, that `header` declares."""
    parsed = header_prototypes(header)
    assert sorted(parsed) == sorted(declared(header))
    ent = {n: a for n, (r, a) in parsed.items() if r is C.c_int and C.c_void_p in a}
    qry = {n: a for n, (r, a) in parsed.items() if r is C.c_longlong}
    return ent, qry


@pytest.mark.parametrize("header", HEADERS)
def test_every_entry_has_a_row(header):
    ent, qry = _entries(header)
    rows = {r.name: r for r in ROWS if r.header == header}
    assert sorted(set(ent) - set(rows) - set(ACCOUNTED_FOR)) == [], "int entries with a pointer parameter and no row"
    assert sorted(set(rows) - set(ent)) == [], "rows of names the header does not declare"
    assert not set(rows) & set(ACCOUNTED_FOR) and all(ACCOUNTED_FOR.values())
    for n, r in rows.items():
        assert r.types == ent[n], f"{n}: the row's parameters {[t.__name__ for t in r.types]} are not the header's"
    queries = {r.name: r for r in QUERIES if r.header == header}
    assert sorted(queries) == sorted(qry), "long long size queries without a row, or rows without a declaration"
    for n, r in queries.items():
        assert r.types == qry[n], n
    for r in rows.values():                                                 # a row's queries exist and fit their arguments
        for qi, (qname, exprs) in enumerate(r.queries):
            assert qname in QUERY and len(exprs.split()) == len(QUERY[qname].types), (r.name, qname)
        used = sorted(p["q"] for p in r.params if p["cls"] == "query")
        assert used == list(range(len(used))) and len(used) <= len(r.queries), r.name


def test_the_census_is_whole():
    names = set()
    for h in HEADERS:
        ent, qry = _entries(h)
        names |= set(ent) | set(qry)
    assert set(ROW) | set(QUERY) | set(ACCOUNTED_FOR) == names and len(ROWS) == len(ROW) and len(QUERIES) == len(QUERY)
    assert all(n in {x for h in HEADERS for x in header_prototypes(h)} for n in INT_CONSTS)


# ---- the contract ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_entry_keeps_the_refusal_contract(name, results):
    bad = classify(ROW[name], results)
    assert not bad, "\n" + _report(bad)


@pytest.mark.parametrize("name", [r.name for r in QUERIES])
def test_size_query_is_zero_for_sizes_it_cannot_serve(name, results):
    bad = classify_query(QUERY[name], results)
    assert not bad, "\n" + _report(bad)
    assert all(v >= 0 or v == QUERY[name].refusal for k, v in results.items() if k.startswith(name + "|"))


def test_the_two_entries_of_test_abi_are_in_the_table(results):
    for name in ("ecm_costvol_concat_fwd", "ecm_conv3d_k3_fwd"):
        assert classify(ROW[name], results) == []


# ---- the classifier can fail: planted defects --------------------------------------------------------------------------------

_FAKE = Row("fake_fwd", "x:p skip:o y:p scratch:p scratch_bytes=Q0 B=1 Ci=4%4 stride=?1 stream:s",
            queries=[("fake_scratch_bytes", "B Ci")], unsup=[{"Ci": 5}, {"stride": 3}])
_SIG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p)
_QSIG = C.CFUNCTYPE(C.c_longlong, C.c_int, C.c_int)


def _fake_query(B, Ci):
    return 64 * B * Ci if B > 0 and Ci > 0 and Ci % 4 == 0 else 0


def _fake(forget_y=False, unsup_as_einval=False, launch_before_scratch=False):
    def f(x, skip, y, scratch, scratch_bytes, B, Ci, stride, stream):
        if not (x and scratch and (y or forget_y) and B > 0 and Ci > 0):
            return EINVAL
        if Ci % 4 or stride < 1 or stride > 2:
            return EINVAL if unsup_as_einval else EUNSUP
        if launch_before_scratch:
            return 100
        if scratch_bytes < _fake_query(B, Ci):
            return ESCRATCH
        return 100
    return f


def _run_fake(**defect):
    fns = {"fake_fwd": _SIG(_fake(**defect)), "fake_scratch_bytes": _QSIG(_fake_query)}
    got = child.execute(calls_of(_FAKE, lambda q: [C.c_int, C.c_int]), lambda name, res, argtypes: fns[name])
    return classify(_FAKE, got)


def test_classifier_passes_a_clean_entry():
    assert _run_fake() == []


@pytest.mark.parametrize("defect,argument,got,want", [
    ("forget_y", "y=NULL", "100", "ECM_EINVAL"),
    ("unsup_as_einval", "Ci=5", "ECM_EINVAL", "ECM_EUNSUP"),
    ("launch_before_scratch", "scratch_bytes=query-1", "100", "ECM_ESCRATCH"),
])
def test_classifier_reports_planted_defect(defect, argument, got, want):
    bad = _run_fake(**{defect: True})
    assert ("fake_fwd", argument, got, want) in bad, bad
    if defect != "unsup_as_einval":
        assert len(bad) == 1, bad
    else:
        assert sorted(a for _, a, _, _ in bad) == ["Ci=5", "stride=-1", "stride=0", "stride=3"]
    assert "fake_fwd: " + argument in _report(bad)
