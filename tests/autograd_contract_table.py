"""The table of tests/test_hip_autograd_contract.py (on the MI355X) and tests/test_autograd_contract_cpu.py (anywhere): what
every torch.autograd.Function of ops.py takes and returns, and the rows that drive it.  Plain data: nothing here imports torch,
the library or a case table -- the GPU file resolves a row's case name in the fp64 suite that owns it.

FUNCTIONS[name] = (tensor parameters of forward, its other parameters, length of every tuple backward returns).
ROWS[id] = Row(functions it is a row for, kind = the builder of the GPU file, case = the name of the shape in that suite's
table (or the shape itself where the issue names one), opts)."""
import collections

FUNCTIONS = {
    "CostVolumeConcat": (("left", "right"), ("ndisp",), 3),
    "CostvolConvAssemble": (("P", "Qp"), ("ndisp",), 3),
    "ClassWeights": (("w",), (), 1),
    "SoftArgminHeads": (("c",), (), 1),
    "ECMAggregate9": (("d", "w9"), ("scale",), 3),
    "ContextWeights": (("lr", "hr", "W0", "W1", "W2", "W3"), ("variant",), 7),
    "VolumeMapping": (("c", "m5", "mt3"), ("scale",), 4),
    "TrilinearSoftArgmin": (("c",), ("Do", "H", "W"), 4),
    "Fork": (("x",), ("n",), 2),
    "ForkHead": (("x",), ("n",), 2),
    "Conv3dK3": (("x", "w"), ("stride", "fork", "grad_mode"), 5),
    "Conv2dG": (("x", "w"), ("stride", "dil", "pad_top", "pad_left", "Ho", "Wo", "fork", "grad_mode"), 10),
    "Conv2dPlanes": (("x", "w"), ("fork", "grad_mode"), 4),
    "Deconv3dK3S2": (("x", "w"), (), 2),
    "Deconv2dK3S2Bias": (("x", "w", "b"), (), 3),
    "Conv2dC1Relu": (("x", "w", "b"), (), 3),
    "GroupNormAct": (("x", "gamma", "beta", "skip"), ("relu", "head"), 6),
    "ClassifierTail": (("x", "gamma", "beta", "w"), (), 4),
    "StereoLoss3": (("p1", "p2", "p3", "gt"), ("maxdisp", "w1", "w2", "w3"), 8),
}

Row = collections.namedtuple("Row", "functions kind case opts", defaults=({},))

ROWS = {}


def _row(rid, functions, kind, case, **opts):
    assert rid not in ROWS, rid
    ROWS[rid] = Row((functions,) if isinstance(functions, str) else tuple(functions), kind, case, opts)


# ---- Conv3dK3: one row per backward branch (tests/test_hip_conv3d_fp64.py's table) ------------------------------------------------
_row("conv3d.c1", "Conv3dK3", "conv3d", "c_ci16")                                  # the 32 -> 1 kernels
_row("conv3d.wino", "Conv3dK3", "conv3d", "w_fork_co40", fork=False)               # Winograd, data-gradient layout packed in forward
_row("conv3d.wino.fork", "Conv3dK3", "conv3d", "w_fork_co40", fork=True)           # ... with the skip gradient in the epilogue
_row("conv3d.direct_s1", "Conv3dK3", "conv3d", "d_s1_t2_small")                    # ops.WINOGRAD off: flip-transposed data gradient
_row("conv3d.direct_s1.fork", "Conv3dK3", "conv3d", "d_s1_t2_small", fork=True)    # ... _fork_grad's plain add
_row("conv3d.s2", "Conv3dK3", "conv3d", "d_s2_t1_small_c2")                        # every extent odd: transposed-conv data gradient
# the split-bf16 stride-2 path (ops.split_products; tests/test_split_bf16_cpu.py's table): its smallest case, one voxel, and the
# smallest whose operands have more than one layout
for _case in ("c_one_voxel", "c_chunk_walk"):
    _row(f"conv3d.split.{_case}", "Conv3dK3", "split", _case, fork=False)
    _row(f"conv3d.split.{_case}.fork", "Conv3dK3", "split", _case, fork=True)
# ---- Conv2dG (tests/test_hip_conv2d_fp64.py's table) ------------------------------------------------------------------------------
for _name, _case in (("wino", "w_ci4_w3"), ("mfma_s1", "m33_c2_small"), ("s2_k3", "ms2_c2_small"), ("s2_k1", "m11s2_c1")):
    _row("conv2d." + _name, "Conv2dG", "conv2d", _case, fork=False)
    _row("conv2d." + _name + ".fork", "Conv2dG", "conv2d", _case, fork=True)
_row("conv2d.class_q", "Conv2dG", "conv2d", "m35_q_small", fork=False)             # asymmetric padding, Wo = W + 2
_row("conv2d_planes", "Conv2dPlanes", "conv2d", "w_planes_p4", fork=False)
_row("conv2d_planes.fork", "Conv2dPlanes", "conv2d", "w_planes_p4", fork=True)
_row("deconv3d", "Deconv3dK3S2", "conv3d", "t_4_32_one_chunk")
_row("deconv2d_bias", "Deconv2dK3S2Bias", "conv2d", "db_4_32_one_chunk")
_row("conv2d_c1_relu", "Conv2dC1Relu", "conv2d", "c1_ci5_w1")
# ---- GroupNormAct: a shape per kernel path of tests/test_hip_groupnorm_fp64.py's table, at B = 2 (the head fork needs two samples)
# x (skip, no skip) x (relu, no relu) x (head 0, head 1).  cluster, one workgroup per channel; cluster, several workgroups per
# channel with a ragged last slice; two-stage by shape (S % 4 = 1); both branches of gn_pivot; two-stage chunking over several
# chunks (cluster mode 0, as the fp64 suite reaches it).
for _shape, _mode in (("w1_part_wave", 1), ("ragged_cpg1", 1), ("s_mod4_1", 1), ("pivot_n15", 1), ("pivot_n17", 1), ("chunk_2p4", 0)):
    for _skip in (False, True):
        for _relu in (False, True):
            for _head in (0, 1):
                _row(f"gn.{_shape}.{'skip' if _skip else 'noskip'}.{'relu' if _relu else 'lin'}.head{_head}", "GroupNormAct", "gn",
                     _shape, skip=_skip, relu=_relu, head=_head, mode=_mode)
_row("classifier_tail", "ClassifierTail", "tail", (1, 32, 3, 5, 6))
_row("cost_volume", "CostVolumeConcat", "costvol", (1, 4, 5, 7, 3))
_row("costvol_conv3d", ("CostvolConvAssemble", "ClassWeights"), "costvol_conv", "cc_w1")       # the smallest: 1 x 1 maps
_row("costvol_conv3d.w9", ("CostvolConvAssemble", "ClassWeights"), "costvol_conv", "cc_w9")    # maps with more than one layout
# ---- the heads and the context mapping: the smallest case per variant of tests/test_hip_context_fp64.py's table --------------------
_row("softargmin_heads", "SoftArgminHeads", "context", "SOFTARGMIN")
_row("ecm_aggregate9", "ECMAggregate9", "context", "AGGREGATE")
for _v in (0, 1, 2):
    _row(f"context_weights.v{_v}", "ContextWeights", "context", "WEIGHTS", variant=_v)
_row("volume_mapping", "VolumeMapping", "context", "VOLUME")
_row("trilinear_softargmin", "TrilinearSoftArgmin", "context", "TRILINEAR")
_row("stereo_loss3", "StereoLoss3", "loss", (1, 1, 9, 14))
for _n in (2, 3, 5):
    for _tag, _shape in (("v4", (2, 8, 3, 5, 6)), ("scalar", (2, 8, 3, 5, 7))):          # numel % 4 == 0 / != 0 (ecm_sum_n)
        _row(f"fork.n{_n}.{_tag}", "Fork", "fork", _shape, n=_n)
for _tag, _shape in (("v4", (2, 8, 3, 5, 6)), ("scalar", (2, 8, 3, 5, 7))):
    _row(f"fork_head.{_tag}", "ForkHead", "fork_head", _shape, n=1)

# Functions whose weight gradient goes through ops._on_side (Conv3dK3: tests/test_hip_wgrad_overlap.py): the rows of V5
ACCUMULATION_ROWS = ("conv2d.wino", "conv2d.mfma_s1", "conv2d_planes", "deconv3d", "classifier_tail")
# ... and the rows whose weight layouts run again with the side stream on (V2)
OVERLAP_ROWS = ACCUMULATION_ROWS + ("conv3d.wino", "conv3d.s2")
# ContextWeights: each input alone, the two maps alone, the four MLP weights alone
CONTEXT_SUBSETS = (("lr",), ("hr",), ("W0",), ("W1",), ("W2",), ("W3",), ("lr", "hr"), ("W0", "W1", "W2", "W3"))


def functions_with_rows():
    return {f for r in ROWS.values() for f in r.functions}
