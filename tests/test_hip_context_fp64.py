"""The context-mapping kernels -- the weight generators (csrc/ecm_weights.hip, ecm_weights_bwd.hip, ecm_nbr.h) and the disparity
heads (csrc/heads.hip, variants.hip) -- against fp64 on every path their host code can take, reached through ecm_amd.ops as the
models reach them: context_weights / ecm_weights9, ecm_aggregate9, softargmin_heads, volume_mapping, trilinear_softargmin and the
autograd of each.

Reference.  The oracle functions of oracle/ecm_oracle.py evaluated in fp64 on the CPU (`offset_tables` follows the dtype of its
caller's input).  Every case of this table is small enough for the oracle itself, O.volume_mapping's python loop over the
disparities included (at most 32 of them here), so the vectorised closed forms -- `planes_t` and `aggregate9_t` below, and volume_mapping_t /
trilinear_t / soft_argmin_t of tests/test_hip_variants_fullsize.py -- serve only as the second fp32 evaluation;
tests/test_context_geometry.py shows on the CPU that each of them equals the oracle in fp64 to 1e-12 of scale.

Yardstick (tests/test_hip_numerics.py's rule, as in the GroupNorm and convolution suites).  For every output and every gradient q,
e32(q) = the largest error against fp64 over two independent fp32 evaluations of the same expression: the oracle in fp32 on the
CPU and the closed form in fp32 on the device.  A kernel passes when  max|q_hip - q64| <= K * e32(q) + FLOOR * max|q64|  with
K = 4, FLOOR = 2e-7.  Each check prints `CMRATIO <path> <quantity> <ratio>`, ratio = error / bound; DESIGN.md section 4 holds the
worst ratio per path and quantity as measured on the MI355X (0.41 over all of them: no path needed a further fp32 candidate in
the kernel's own summation order).

LeakyReLU kinks (weights backward only).  The forward is continuous; the backward's mask is not, and a correct fp32 evaluation
may flip it where a pre-activation is near zero.  A pixel is "at a kink" when any fp64 pre-activation (32 + 16 + 8 layer values,
plus the final one for the six-related variants) of the MLP of any of its in-image neighbours lies within KINK_EPS = 1e-5 of
zero: 4x the fp32 pre-activation error of 2.1e-6 .. 2.5e-6 measured on the CPU at (B,h,w,s) = (1,3,9,8), (1,2,5,16), (2,5,33,4).
The gradient handed to backward is zero at those pixels on all planes, so such a pixel contributes nothing to any gradient; that
is the only exclusion, and the share of such pixels is at most KINK_SHARE = 0.5 % in every case (asserted here and, on the CPU,
in tests/test_context_geometry.py; the operand names carry a per-case salt chosen so that it holds).

Reproducibility and stale memory.  Every case runs twice on fresh copies of its operands and all outputs must match bit for bit
(the kernels claim fixed-order sums).  Operands differ between cases, a case's outputs stay alive until it ends, and before each
run the caching allocator's unused blocks go back to the driver and fresh ones are filled with NaN and freed (`poison`), so that an
element a kernel fails to write -- in an output or in its scratch -- cannot inherit the right value from recycled memory.

Case table.  `bwd_plan`, `fwd_geom` and the `*_grid` functions restate the host-side dispatch; `classes_of` lists the path
classes a case reaches and `missing_classes()` must be empty (tests/test_context_geometry.py pins the constants to the sources).
Every case is the smallest shape that reaches its classes; the two that make workgroups of ecm_weights_bwd_kernel_p walk two
tiles need 520 tiles of 4 x 64 pixels (an `hr` tensor of 17 MB)."""
import collections
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import oracle.ecm_oracle as O
from oracle.weights import seeded, tensor_for
from test_hip_conv3d_fp64 import DEV, FLOOR, K, cdiv
from test_hip_variants_fullsize import soft_argmin_t, trilinear_t, volume_mapping_t

pytestmark = pytest.mark.gpu

KINK_EPS, KINK_SHARE = 1e-5, 0.005

# ---- constants of the sources (tests/test_context_geometry.py pins them) -----------------------------------------------------------
CF, TX, TY = 32, 64, 4                  # ecm_weights.hip, ecm_weights_bwd.hip: channels, pixels of a tile
NCXMAX, UST, PB_N = TX // 4 + 2, 48, 1736
MAX_WORKERS = 512                       # plan(): workgroups of ecm_weights_bwd_kernel_p
CELL_BLOCK = 128                        # cells per workgroup of ecm_weights_bwd_cells
BWD_SCALES = (4, 8, 16)                 # the backward's gate
THREADS, ROWS_PER_WG = 256, 4           # heads.hip / variants.hip: one thread per element; 4 waves = 4 cells / 4 rows per workgroup
# ecm_nbr.h: (dy, dx, table) per plane
NBR = {0: ((0, 0, 0), (0, -1, 1), (0, 1, 2), (-1, 0, 3), (1, 0, 4), (-1, -1, 1), (-1, 1, 2), (1, -1, 3), (1, 1, 4)),
       1: ((0, 0, 0), (0, 1, 1), (0, -1, 2), (-1, 0, 3), (1, 0, 4)),
       2: ((0, 0, 0), (0, 1, 1), (0, -1, 2))}
PAIRS = ((0, 4), (1, 4), (1, 8), (1, 16), (2, 4), (2, 8), (2, 16))       # (variant, scale) with a backward
RAGGED = {4: (4,), 8: (8,), 16: (16, 48)}                                # W % 64 of the ragged right tile, per scale
MLP_KEYS = [f"mapping_matrix.similarity1.conv{i}.weight" for i in range(4)]
MLP_SHAPES = ((32, 66, 1, 1), (16, 32, 1, 1), (8, 16, 1, 1), (1, 8, 1, 1))


# ---- host-side dispatch, restated ------------------------------------------------------------------------------------------------
def bwd_plan(B, h, w, s):
    """plan() of ecm_weights_bwd.hip and the per-wave cell geometry of ecm_weights_bwd_kernel_p."""
    tiles_x, rbs = cdiv(w * s, TX), h * s // TY
    ntiles = B * rbs * tiles_x
    return dict(tiles_x=tiles_x, rbs=rbs, ntiles=ntiles, nB=min(ntiles, MAX_WORKERS), nC=cdiv(B * h * w, CELL_BLOCK), rpc=s // TY,
                lpc=4 * s)


def fwd_geom(B, h, w, s):
    """Grid of ecm_weights_fwd_kernel and the LR cell window (cy0, cx0, ncy, ncx) of each of its tiles."""
    H, W = h * s, w * s
    grid = (cdiv(W, TX), cdiv(H, TY), B)
    win = {}
    for ty in range(grid[1]):
        for tx in range(grid[0]):
            Y0, X0 = ty * TY, tx * TX
            win[ty, tx] = (Y0 // s - 1, X0 // s - 1, (Y0 + TY - 1) // s - Y0 // s + 3, (X0 + TX - 1) // s - X0 // s + 3)
    return grid, win


def fwd_lds_cells(s):
    return ((TY - 1) // s + 4) * ((TX - 1) // s + 4)


def softargmin_grid(B, h, w):
    return cdiv(B * h * w, THREADS)


def aggregate_grids(B, h, w, s):
    """(pixels kernel, gather kernel: one wave per LR cell, its 64 lanes over 9 s^2 items)."""
    return cdiv(B * h * s * w * s, THREADS), cdiv(B * h * w, ROWS_PER_WG)


def volume_grids(B, h, w, s):
    """(forward, backward: one wave per image row, gather); the backward walks a row in chunks of 64 columns."""
    return cdiv(B * h * s * w * s, THREADS), cdiv(B * h * s, ROWS_PER_WG), cdiv(w * s, 64)


def trilinear_grid(B, H, W):
    return cdiv(B * H * W, THREADS)


def tri_src(dst, scale, n):
    """src_index of variants.hip (PyTorch's align_corners=False rule): the two source planes of output index dst."""
    src = max(scale * (dst + 0.5) - 0.5, 0.0)
    i0 = min(int(src), n - 1)
    return i0, i0 + (1 if i0 < n - 1 else 0)


def reduce_bucket(n):
    """Which loops of ecm_weights_bwd_reduce a partial count n runs."""
    if n < 8:
        return "idle-groups"
    if n <= 24:
        return "tail-loop-only"
    return "unrolled-edge" if (n - 24) % 32 < 8 else "unrolled"       # edge: a lane group's 4th stride lands on index n exactly


# ---- case tables -----------------------------------------------------------------------------------------------------------------
WCase = collections.namedtuple("WCase", "variant B h w s grads", defaults=(True,))
SCase = collections.namedtuple("SCase", "NH B D h w scale")                       # softargmin_heads
ACase = collections.namedtuple("ACase", "NH B h w s")                             # ecm_aggregate9
VCase = collections.namedtuple("VCase", "NH B Dl h w s")                          # volume_mapping
TCase = collections.namedtuple("TCase", "NH B Dl h w Do H W")                     # trilinear_softargmin

WEIGHTS = {}
for _v in (0, 1, 2):
    WEIGHTS[f"w{_v}s4_exact_h1"] = WCase(_v, 1, 1, 16, 4)                          # one exact tile, 1 partial
    WEIGHTS[f"w{_v}s4_ragged"] = WCase(_v, 2, 3, 17, 4)                            # W = 68: three of a wave's four cells dead
for _v in (1, 2):
    WEIGHTS[f"w{_v}s8_exact"] = WCase(_v, 1, 2, 8, 8)
    WEIGHTS[f"w{_v}s16_exact_h1"] = WCase(_v, 1, 1, 4, 16)
    WEIGHTS[f"w{_v}s16_ragged16"] = WCase(_v, 1, 2, 5, 16)                         # W = 80: waves 1-3 of the last tile dead
    WEIGHTS[f"w{_v}s16_ragged48"] = WCase(_v, 2, 1, 7, 16)                         # W = 112: wave 3 dead
WEIGHTS.update({
    "w1s8_ragged_30": WCase(1, 1, 3, 33, 8),           # W = 264, 30 partials: a lane group's unrolled stride ends on index n
    "w2s8_ragged_24": WCase(2, 1, 3, 25, 8),           # W = 200, 24 partials: the largest count the unrolled loop must not enter
    "w0s4_w1": WCase(0, 1, 3, 1, 4), "w1s8_w1": WCase(1, 1, 3, 1, 8), "w2s16_w1": WCase(2, 1, 2, 1, 16),
    "w1s4_mid": WCase(1, 1, 16, 64, 4),                # 64 tile partials (unrolled), 8 cell partials (tail loop)
    "w0s4_walk": WCase(0, 2, 20, 208, 4),              # 520 tiles on 512 workgroups, 65 cell partials
    "w2s16_walk": WCase(2, 1, 13, 40, 16),             # 520 tiles; 520 cells = 4 blocks + 8
    "w1s2_fwd": WCase(1, 1, 3, 37, 2, False), "w2s2_fwd": WCase(2, 2, 3, 35, 2, False),       # H % 4 == 2
    "w1s6_fwd": WCase(1, 1, 2, 12, 6, False), "w2s6_fwd": WCase(2, 2, 1, 11, 6, False),       # the tile at X0 = 64 starts mid-cell
})
SOFTARGMIN = {"sa_small": SCase(1, 1, 5, 3, 7, 1.5), "sa_ragged": SCase(3, 2, 6, 11, 13, 1.5), "sa_d1": SCase(2, 1, 1, 4, 5, 1.5),
              "sa_scale30": SCase(2, 1, 9, 5, 9, 30.0)}
AGGREGATE = {"ag_s2": ACase(2, 1, 3, 5, 2), "ag_s4": ACase(3, 2, 5, 7, 4), "ag_s8": ACase(1, 1, 2, 3, 8), "ag_s16": ACase(2, 1, 2, 2, 16),
             "ag_h1": ACase(1, 1, 1, 6, 4), "ag_w1": ACase(3, 2, 3, 1, 4)}
VOLUME = {"vm_s4_wide": VCase(3, 1, 3, 3, 19, 4), "vm_s8": VCase(2, 2, 2, 2, 5, 8), "vm_s16_h1": VCase(1, 1, 1, 1, 5, 16),
          "vm_ones_w1": VCase(2, 2, 2, 3, 1, 4), "vm_s2": VCase(3, 1, 2, 3, 5, 2)}
TRILINEAR = {"tl_up4": TCase(3, 1, 3, 3, 4, 12, 12, 16), "tl_up16": TCase(1, 1, 2, 2, 3, 32, 32, 48),
             "tl_nonint": TCase(2, 2, 5, 3, 4, 13, 8, 11), "tl_identity": TCase(2, 1, 4, 5, 6, 16, 5, 6),
             "tl_down": TCase(3, 1, 8, 3, 4, 2, 6, 8), "tl_dl1": TCase(2, 1, 1, 2, 3, 4, 8, 12),
             "tl_h1": TCase(1, 2, 3, 1, 4, 6, 3, 8), "tl_w1": TCase(3, 1, 2, 3, 1, 4, 6, 5)}
# per-case salt of the operand names (module docstring: the kink share), for the cases that miss the cap at salt 0
SALTS = {"w1s8_w1": 1}
CASES = {**WEIGHTS, **SOFTARGMIN, **AGGREGATE, **VOLUME, **TRILINEAR}


def classes_of(c):
    """The path classes one case reaches."""
    out = set()
    if isinstance(c, WCase):
        v, B, h, w, s = c[:5]
        H, W = h * s, w * s
        pair = (v, s)
        grid, win = fwd_geom(B, h, w, s)
        assert all(ncy * ncx <= fwd_lds_cells(s) for _, _, ncy, ncx in win.values())
        if W % TX:
            out.add(("fwd", pair, "ragged-x"))
        if s == 2 and H % TY == 2 and any(ty * TY // s + 1 < h for ty in range(grid[1])):          # both cell rows of the tile in the image
            out |= {("fwd", v, "s2-tile-spans-two-cell-rows"), ("fwd", "Y>=H")}
        if s == 6 and W > TX and any((tx * TX) % s for tx in range(grid[0])):
            out.add(("fwd", v, "s6-tile-starts-mid-cell"))
        if h >= 2 and w >= 2:
            out.add(("fwd", v, "border-planes"))
        if not c.grads:
            out.add(("bwd", v, "refused-scale"))
            assert s not in BWD_SCALES
            return out
        assert pair in PAIRS
        p = bwd_plan(B, h, w, s)
        assert TX // s + 2 <= NCXMAX and 4 * PB_N <= 4 * 64 * UST
        out.add(("bwd", pair, "cell-sum-%d-lanes" % p["lpc"]))
        out.add(("cells", "rpc%d" % p["rpc"]))
        if W == TX:
            out.add(("bwd", pair, "one-exact-tile"))
        if p["tiles_x"] >= 2 and w >= 2:
            out.add(("bwd", pair, "halo-across-tiles"))
        if W > TX and W % TX in RAGGED[s]:
            live = W % TX
            out.add(("bwd", pair, "ragged-%d" % live))
            if live % 16 and s < 16:
                out.add(("bwd", pair, "live-and-dead-cells-in-a-wave"))
            if live <= 48 and s == 16:
                out.add(("bwd", pair, "dead-waves-%d" % ((TX - live) // 16)))
        for flag, nm in ((h == 1, "h1"), (w == 1, "w1"), (B >= 2, "B2")):
            if flag:
                out.add(("bwd", v, nm))
        if p["ntiles"] <= MAX_WORKERS:
            out.add(("bwd", "one-tile-per-workgroup"))
        elif p["ntiles"] % MAX_WORKERS:
            out.add(("bwd", "v0" if v == 0 else "six-s16" if s == 16 else "six", "one-and-two-tiles-per-workgroup"))
        for nm in ("nB", "nC"):
            out.add(("reduce", nm, reduce_bucket(p[nm])))
            if v and reduce_bucket(p[nm]).startswith("unrolled"):
                out.add(("reduce", "six-related", "unrolled"))
        if p["nB"] == MAX_WORKERS:
            out.add(("reduce", "nB", "512"))
        cells = B * h * w
        if p["nC"] == 1 and cells < CELL_BLOCK:
            out.add(("cells", "one-partial-block"))
        if p["nC"] > 1 and cells % CELL_BLOCK:
            out.add(("cells", "blocks-and-a-partial-last"))
    elif isinstance(c, SCase):
        n = c.B * c.h * c.w
        out.add(("softargmin", "NH%d" % c.NH))
        out.add(("softargmin", "below-256" if n < THREADS else "above-256-ragged" if n % THREADS else "multiple"))
        assert softargmin_grid(c.B, c.h, c.w) == (1 if n < THREADS else cdiv(n, THREADS))
        if c.D == 1:
            out.add(("softargmin", "D1"))
        if c.scale >= 30:
            out.add(("softargmin", "scale30"))
    elif isinstance(c, ACase):
        out |= {("aggregate", "NH%d" % c.NH), ("aggregate", "s%d" % c.s)}
        if 9 * c.s * c.s < 64:
            out.add(("aggregate", "idle-gather-lanes"))
        if (c.B * c.h * c.w) % ROWS_PER_WG:
            out.add(("aggregate", "cells%4"))
        assert aggregate_grids(c.B, c.h, c.w, c.s)[1] * ROWS_PER_WG >= c.B * c.h * c.w
        out |= {("aggregate", nm) for flag, nm in ((c.h == 1, "h1"), (c.w == 1, "w1")) if flag}
    elif isinstance(c, VCase):
        W, D = c.w * c.s, c.Dl * c.s
        out |= {("volume", "NH%d" % c.NH), ("volume", "s%d" % c.s), ("volume", "ones-branch" if D > W else "no-ones-branch")}
        _, rows, chunks = volume_grids(c.B, c.h, c.w, c.s)
        assert 4 * 3 * W * 4 <= 160 * 1024 and c.s & (c.s - 1) == 0
        if W < 64:
            out.add(("volume", "W<64"))
        if chunks >= 2 and W % 64:
            out.add(("volume", "chunks-ragged"))
        if (c.B * c.h * c.s) % ROWS_PER_WG:
            out.add(("volume", "BH%4"))
        out |= {("volume", nm) for flag, nm in ((c.Dl == 1, "Dl1"), (c.Dl == 2, "Dl2"), (c.h == 1, "h1"), (c.w == 1, "w1")) if flag}
    elif isinstance(c, TCase):
        out.add(("trilinear", "NH%d" % c.NH))
        for up in (4, 16):
            if (c.Do, c.H, c.W) == (up * c.Dl, up * c.h, up * c.w):
                out.add(("trilinear", "up%d" % up))
        if c.Do % c.Dl and c.H % c.h and c.W % c.w and c.Do > c.Dl:
            out.add(("trilinear", "non-integer-DHW"))
        if (c.H, c.W) == (c.h, c.w):
            out.add(("trilinear", "identity-HW"))
        if c.Do < c.Dl and unsampled_planes(c) and max(unsampled_planes(c)) == c.Dl - 1 and min(unsampled_planes(c)) < c.Dl - 2:
            out.add(("trilinear", "Do<Dl-skipped-and-tail-planes"))
        out |= {("trilinear", nm) for flag, nm in ((c.Dl == 1, "Dl1"), (c.h == 1, "h1"), (c.w == 1, "w1")) if flag}
    return out


def unsampled_planes(c):
    used = set()
    for D in range(c.Do):
        used |= set(tri_src(D, c.Dl / c.Do, c.Dl))
    return sorted(set(range(c.Dl)) - used)


def required_classes():
    req = set()
    for v, s in PAIRS:
        pair = (v, s)
        req |= {("fwd", pair, "ragged-x"), ("bwd", pair, "cell-sum-%d-lanes" % (4 * s)), ("bwd", pair, "one-exact-tile"),
                ("bwd", pair, "halo-across-tiles")}
        req |= {("bwd", pair, "ragged-%d" % r) for r in RAGGED[s]}
        if s < 16:
            req.add(("bwd", pair, "live-and-dead-cells-in-a-wave"))
        else:
            req |= {("bwd", pair, "dead-waves-3"), ("bwd", pair, "dead-waves-1")}
    for v in (0, 1, 2):
        req |= {("bwd", v, "h1"), ("bwd", v, "w1"), ("bwd", v, "B2"), ("fwd", v, "border-planes")}
    for v in (1, 2):
        req |= {("fwd", v, "s2-tile-spans-two-cell-rows"), ("fwd", v, "s6-tile-starts-mid-cell"), ("bwd", v, "refused-scale")}
    req |= {("fwd", "Y>=H"), ("bwd", "one-tile-per-workgroup"), ("bwd", "v0", "one-and-two-tiles-per-workgroup"),
            ("bwd", "six-s16", "one-and-two-tiles-per-workgroup"), ("reduce", "six-related", "unrolled"), ("reduce", "nB", "512"),
            ("reduce", "nB", "unrolled-edge"), ("cells", "one-partial-block"), ("cells", "blocks-and-a-partial-last")}
    req |= {("reduce", nm, b) for nm in ("nB", "nC") for b in ("idle-groups", "tail-loop-only", "unrolled")}
    req |= {("cells", "rpc%d" % r) for r in (1, 2, 4)}
    for fam in ("softargmin", "aggregate", "volume", "trilinear"):
        req |= {(fam, "NH%d" % n) for n in (1, 2, 3)}
    req |= {("softargmin", x) for x in ("below-256", "above-256-ragged", "D1", "scale30")}
    req |= {("aggregate", x) for x in ("s2", "s4", "s8", "s16", "idle-gather-lanes", "cells%4", "h1", "w1")}
    req |= {("volume", x) for x in ("s4", "s8", "s16", "W<64", "chunks-ragged", "ones-branch", "no-ones-branch", "Dl1", "Dl2", "BH%4",
                                    "h1", "w1")}
    req |= {("trilinear", x) for x in ("up4", "up16", "non-integer-DHW", "identity-HW", "Do<Dl-skipped-and-tail-planes", "Dl1", "h1",
                                       "w1")}
    return req


def missing_classes(cases=None):
    cases = CASES if cases is None else cases
    have = set()
    for c in cases.values():
        have |= classes_of(c)
    return sorted(required_classes() - have, key=str)


def smallest_case_per_class():
    """{class: name of the smallest case (by elements of its largest operand) that reaches it}."""
    def size(c):
        if isinstance(c, WCase):
            return c.B * c.h * c.w * c.s * c.s
        return math.prod(c[1:])
    best = {}
    for name, c in CASES.items():
        for cl in classes_of(c):
            if cl not in best or size(c) < size(CASES[best[cl]]):
                best[cl] = name
    return best


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def planes_t(lr, hr, W0, W1, W2, W3, variant, want_pre=False):
    """The three weight generators, vectorised for any dtype / device: the first layer split as the kernels split it (a projection
    per LR cell, one per pixel, two offset columns per neighbour), out-of-image neighbours at the variant's padding logit.
    want_pre: also the smallest |pre-activation| per pixel over all layers of all in-image neighbours, [B,H,W]."""
    B, _, h, w = lr.shape
    H, Wd = hr.shape[-2:]
    s = Wd // w
    dev_, dt = lr.device, lr.dtype
    pad, final = (O.PAD_LOGIT, False) if variant == 0 else (0.0, True)
    w0 = W0.view(32, 66)
    A = torch.einsum("oc,bchw->bohw", w0[:, :32], lr)
    Bv = torch.einsum("oc,bchw->bohw", w0[:, 32:64], hr)
    r = torch.arange(s, device=dev_)
    half = torch.where(r < s // 2, r - s // 2, r - s // 2 + 1).to(dt)
    dn, up = (s - r).to(dt), (r + 1).to(dt)
    X, Y = torch.arange(Wd, device=dev_) % s, torch.arange(H, device=dev_) % s
    Ap = F.pad(A, (1, 1, 1, 1))
    ok = F.pad(torch.ones(1, 1, h, w, device=dev_, dtype=dt), (1, 1, 1, 1))
    leaky = lambda t: F.leaky_relu(t, O.LEAKY)                               # noqa: E731
    logits, near = [], None
    for dy, dx, t in NBR[variant]:
        offx = (dn if t == 1 else up if t == 2 else half)[X].view(1, 1, 1, Wd)
        offy = (dn if t == 3 else up if t == 4 else half)[Y].view(1, 1, H, 1)
        a = Ap[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w].repeat_interleave(s, -1).repeat_interleave(s, -2)
        valid = ok[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w].repeat_interleave(s, -1).repeat_interleave(s, -2)
        p0 = a + Bv + w0[:, 64].view(1, 32, 1, 1) * offx + w0[:, 65].view(1, 32, 1, 1) * offy
        p1 = torch.einsum("oc,bchw->bohw", W1.view(16, 32), leaky(p0))
        p2 = torch.einsum("oc,bchw->bohw", W2.view(8, 16), leaky(p1))
        p3 = torch.einsum("oc,bchw->bohw", W3.view(1, 8), leaky(p2))
        z = leaky(p3) if final else p3
        logits.append(z * valid + pad * (1 - valid))
        if want_pre:
            m = torch.cat([p0, p1, p2] + ([p3] if final else []), 1).detach().abs().amin(1, keepdim=True)
            m = torch.where(valid > 0, m, torch.full_like(m, float("inf")))
            near = m if near is None else torch.minimum(near, m)
    allp = torch.cat(logits, 1)
    out = F.softmax(allp, 1) * allp if variant else F.softmax(allp, 1)
    return (out, near[:, 0]) if want_pre else out


def aggregate9_t(d, w9, s):
    """cmfsm.py:709-723 for all heads at once: d [NH,B,h,w], w9 [B,9,H,W] -> [NH,B,H,W]; a zero border stands for the
    neighbours outside the image."""
    h, w = d.shape[-2:]
    dp = F.pad(d, (1, 1, 1, 1)) * s
    out = 0
    for n, (dy, dx, _) in enumerate(NBR[0]):
        nb = dp[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w].repeat_interleave(s, -1).repeat_interleave(s, -2)
        out = out + nb * w9[:, n].unsqueeze(0)
    return out


def outside_mask(variant, B, h, w, s):
    """[B,N,H,W] bool: plane n's neighbour cell lies outside the image."""
    cy = torch.arange(h * s).view(-1, 1) // s
    cx = torch.arange(w * s).view(1, -1) // s
    m = [((cy + dy < 0) | (cy + dy >= h) | (cx + dx < 0) | (cx + dx >= w)) for dy, dx, _ in NBR[variant]]
    return torch.stack(m, 0).unsqueeze(0).expand(B, -1, -1, -1)


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def mlp_weights():
    return [tensor_for(k, sh) for k, sh in zip(MLP_KEYS, MLP_SHAPES)]


def _nm(name):
    return f"cm.{name}.{SALTS.get(name, 0)}"


@functools.lru_cache(maxsize=None)
def kink(name):
    """(keep [B,1,H,W] fp32: 0 at the pixels at a LeakyReLU kink, share of such pixels), in fp64 on the CPU."""
    c = CASES[name]
    o = _weights_inputs(name, c)
    _, near = planes_t(o["lr"].double(), o["hr"].double(), *[t.double() for t in mlp_weights()], c.variant, want_pre=True)
    at = near < KINK_EPS
    return (~at).float().unsqueeze(1), float(at.double().mean())


def _weights_inputs(name, c):
    n = _nm(name)
    return {"lr": seeded(n + ".lr", c.B, CF, c.h, c.w), "hr": seeded(n + ".hr", c.B, CF, c.h * c.s, c.w * c.s)}


def operands(name):
    c, n = CASES[name], _nm(name)
    if isinstance(c, WCase):
        o = _weights_inputs(name, c)
        o.update({"W%d" % i: t for i, t in enumerate(mlp_weights())})
        if c.grads:
            o["G"] = seeded(n + ".G", c.B, len(NBR[c.variant]), c.h * c.s, c.w * c.s) * kink(name)[0]
        return o
    if isinstance(c, SCase):
        return {"c": seeded(n + ".c", c.NH, c.B, c.D, c.h, c.w, scale=c.scale), "G": seeded(n + ".G", c.NH, c.B, c.h, c.w)}
    if isinstance(c, ACase):
        return {"d": seeded(n + ".d", c.NH, c.B, c.h, c.w, scale=10.0),
                "w9": torch.softmax(seeded(n + ".w", c.B, 9, c.h * c.s, c.w * c.s), 1), "G": seeded(n + ".G", c.NH, c.B, c.h * c.s, c.w * c.s)}
    if isinstance(c, VCase):
        H, W = c.h * c.s, c.w * c.s
        return {"c": seeded(n + ".c", c.NH, c.B, c.Dl, c.h, c.w, scale=1.5), "m5": seeded(n + ".m5", c.B, 5, H, W, scale=0.5),
                "mt3": seeded(n + ".mt3", c.B, 3, H, W, scale=0.5), "G": seeded(n + ".G", c.NH, c.B, H, W)}
    return {"c": seeded(n + ".c", c.NH, c.B, c.Dl, c.h, c.w, scale=1.5), "G": seeded(n + ".G", c.NH, c.B, c.H, c.W)}


INPUTS = {WCase: ("lr", "hr", "W0", "W1", "W2", "W3"), SCase: ("c",), ACase: ("d", "w9"), VCase: ("c", "m5", "mt3"), TCase: ("c",)}
GRADS = {WCase: ("glr", "ghr", "gW0", "gW1", "gW2", "gW3"), SCase: ("gc",), ACase: ("gd", "gw9"), VCase: ("gc", "gm5", "gmt3"),
         TCase: ("gc",)}


def path_of(c):
    if isinstance(c, WCase):
        return f"weights.v{c.variant}.s{c.s}"
    if isinstance(c, (ACase, VCase)):
        return f"{'aggregate9' if isinstance(c, ACase) else 'volume_mapping'}.s{c.s}"
    return "softargmin" if isinstance(c, SCase) else "trilinear"


# ---- evaluations -------------------------------------------------------------------------------------------------------------------
def _heads(fn, c, NH):
    """Head k of the models takes the logits c_0 + ... + c_k."""
    return torch.stack([fn(c[:k + 1].sum(0)) for k in range(NH)], 0)


def evaluate(c, o, dtype, device, closed):
    """{quantity: tensor} of one case by the oracle (closed=False, CPU only where it builds CPU tensors) or the closed forms."""
    ins = [o[k].to(device=device, dtype=dtype, copy=True) for k in INPUTS[type(c)]]
    grads = not isinstance(c, WCase) or c.grads
    if grads:
        ins = [t.requires_grad_() for t in ins]
    if isinstance(c, WCase):
        if closed:
            y = planes_t(*ins, c.variant)
        else:
            sd = dict(zip(MLP_KEYS, ins[2:]))
            y = (O.ecm_weights_eight(ins[0], ins[1], sd) if c.variant == 0 else
                 O._six_planes(ins[0], ins[1], sd, "mapping_matrix.similarity1", O.SIX_LEFT if c.variant == 1 else O.SIX_RIGHT))
    elif isinstance(c, SCase):
        y = _heads(soft_argmin_t if closed else O.soft_argmin, ins[0], c.NH)
    elif isinstance(c, ACase):
        y = aggregate9_t(ins[0], ins[1], c.s) if closed else torch.stack([O.ecm_aggregate_eight(ins[0][k], ins[1], c.s)[:, 0] for k in range(c.NH)], 0)
    elif isinstance(c, VCase):
        fn = (lambda t: volume_mapping_t(t, ins[1], ins[2], c.s)) if closed else (lambda t: O.volume_mapping(t, ins[1], ins[2], c.s, c.Dl * c.s))
        y = _heads(fn, ins[0], c.NH)
    else:
        y = _heads((lambda t: trilinear_t(t, c.Do, c.H, c.W)) if closed else (lambda t: O.trilinear_head(t, c.Do, c.H, c.W)), ins[0], c.NH)
    out = {"out": y.detach()}
    if grads:
        y.backward(o["G"].to(device=device, dtype=dtype))
        out.update({g: t.grad for g, t in zip(GRADS[type(c)], ins)})
    return out


def poison():
    """Fill what the caching allocator will hand out next with NaN: its unused blocks go back to the driver, then one large block
    and a run of small ones are filled and freed -- the only free blocks it then has."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 26,), float("nan"), device=DEV)] + [torch.full((1 << 16,), float("nan"), device=DEV) for _ in range(64)]
    del junk


def hip(ecm, c, o):
    ops = ecm.ops
    poison()
    ins = [o[k].to(DEV) for k in INPUTS[type(c)]]
    grads = not isinstance(c, WCase) or c.grads
    if grads:
        ins = [t.requires_grad_() for t in ins]
    if isinstance(c, WCase):
        y = ops.ecm_weights9(*ins) if c.variant == 0 else ops.context_weights(*ins, c.variant)
    elif isinstance(c, SCase):
        y = ops.softargmin_heads(ins[0])
    elif isinstance(c, ACase):
        y = ops.ecm_aggregate9(ins[0], ins[1], c.s)
    elif isinstance(c, VCase):
        y = ops.volume_mapping(*ins, c.s)
    else:
        y = ops.trilinear_softargmin(ins[0], c.Do, c.H, c.W)
    out = {"out": y.detach()}
    if grads:
        y.backward(o["G"].to(DEV))
        out.update({g: t.grad for g, t in zip(GRADS[type(c)], ins)})
    elif isinstance(c, WCase):
        ins = [t.requires_grad_() for t in ins]
        y = ops.context_weights(*ins, c.variant)
        with pytest.raises(RuntimeError, match="context_weights backward: unsupported scale"):
            y.backward(torch.ones_like(y))
    shapes = {"out": y.shape, **{g: o[k].shape for g, k in zip(GRADS[type(c)], INPUTS[type(c)])}}
    for k, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == shapes[k], k
    return out


def structure_checks(name, c, a, q64, fails):
    """What a case's outputs must satisfy exactly, beyond the bound."""
    if isinstance(c, WCase):
        out = a["out"].cpu()
        outside = outside_mask(c.variant, c.B, c.h, c.w, c.s)
        if c.variant == 0:
            dev1 = float((out.double().sum(1) - 1).abs().max())
            if dev1 > 9 * 2.0 ** -23:                              # nine roundings of a value <= 1
                fails.append(f"{name}: the nine planes sum to 1 +- {dev1:.2e}")
            # out-of-image planes: exp(-100 - max) / sum -- an fp32 denormal (or zero, where the device flushes them)
            v, r = out[outside].double(), q64["out"][outside]
            if v.numel() and not bool(((v >= 0) & (v <= 2 * r + 2.0 ** -149)).all()):
                fails.append(f"{name}: out-of-image planes are not exp(-100 - max)/sum: max {float(v.max()):.3e} vs {float(r.max()):.3e}")
        elif outside.any() and not bool((out[outside] == 0).all()):          # logit 0: softmax * 0, yet still in the softmax
            fails.append(f"{name}: out-of-image planes of the six-related variant are not exactly zero")
    if isinstance(c, TCase) and unsampled_planes(c):
        j = unsampled_planes(c)
        if not bool((a["gc"][:, :, j] == 0).all()) or not bool((q64["gc"][:, :, j] == 0).all()):
            fails.append(f"{name}: the gradient of the unsampled planes {j} is not exactly zero")


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


def run_case(ecm, name):
    c = CASES[name]
    if isinstance(c, WCase) and c.grads:
        share = kink(name)[1]
        print(f"CMKINK {name} {share:.5f}")
        assert share <= KINK_SHARE, f"{name}: {share:.3%} of the pixels lie within {KINK_EPS} of a LeakyReLU kink"
    o = operands(name)
    fails, runs = [], None
    try:
        runs = [hip(ecm, c, o) for _ in range(2)]
        a, b = runs
        q64 = evaluate(c, o, torch.float64, "cpu", False)
        draws = [evaluate(c, o, torch.float32, "cpu", False), evaluate(c, o, torch.float32, DEV, True)]
        assert set(a) == set(q64)
        for k, got in a.items():
            ref = q64[k]
            each = [float((d[k].cpu().double() - ref).abs().max()) for d in draws]
            e32, scale = max(each), float(ref.abs().max())
            err = float((got.cpu().double() - ref).abs().max())
            bound = K * e32 + FLOOR * scale
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            print(f"CMRATIO {path_of(c)} {k} {ratio:.3f}   # {name}: err {err:.3e}, e32 {e32:.3e} [{each[0]:.2e} {each[1]:.2e}], max|ref| {scale:.3e}")
            if not err <= bound:                                     # (a NaN fails)
                fails.append(f"{name}: {k} on {path_of(c)}: |hip - fp64| = {err:.3e} > {K} * {e32:.3e} + {FLOOR} * {scale:.3e} (ratio {ratio:.2f})")
            if not torch.equal(got, b[k]):
                fails.append(f"{name}: {k} differs between two runs in {int((got != b[k]).sum())} elements")
        structure_checks(name, c, a, q64, fails)
        ecm.ops.check_async_errors()
        assert not fails, "\n".join(fails)
    finally:
        del runs


# ---- the closed forms are the oracle (called on the CPU by tests/test_context_geometry.py) -----------------------------------------
def closed_form_gaps():
    """{name: max|closed form - oracle| / max|oracle|} in fp64, outputs and gradients, at small shapes with every border."""
    gaps = {}
    shapes = [WCase(0, 2, 3, 4, 4), WCase(0, 1, 2, 1, 4), WCase(1, 1, 2, 3, 8), WCase(2, 2, 2, 3, 4), WCase(1, 1, 3, 2, 6), WCase(2, 1, 1, 2, 16),
              SCase(3, 2, 7, 3, 4, 30.0), ACase(3, 2, 3, 4, 4), ACase(2, 1, 1, 3, 2), ACase(1, 1, 2, 1, 8), VCase(2, 2, 3, 2, 3, 4), VCase(3, 1, 2, 1, 2, 8), VCase(1, 1, 2, 2, 1, 2),
              TCase(2, 2, 5, 3, 4, 13, 8, 11), TCase(3, 1, 8, 3, 4, 2, 6, 8)]
    for i, c in enumerate(shapes):
        n = f"cm.closed{i}"
        if isinstance(c, WCase):
            o = {"lr": seeded(n + ".lr", c.B, CF, c.h, c.w), "hr": seeded(n + ".hr", c.B, CF, c.h * c.s, c.w * c.s),
                 "G": seeded(n + ".G", c.B, len(NBR[c.variant]), c.h * c.s, c.w * c.s)}
            o.update({"W%d" % j: t for j, t in enumerate(mlp_weights())})
        elif isinstance(c, SCase):
            o = {"c": seeded(n + ".c", c.NH, c.B, c.D, c.h, c.w, scale=c.scale), "G": seeded(n + ".G", c.NH, c.B, c.h, c.w)}
        elif isinstance(c, ACase):
            o = {"d": seeded(n + ".d", c.NH, c.B, c.h, c.w, scale=10.0), "w9": torch.softmax(seeded(n + ".w", c.B, 9, c.h * c.s, c.w * c.s), 1),
                 "G": seeded(n + ".G", c.NH, c.B, c.h * c.s, c.w * c.s)}
        elif isinstance(c, VCase):
            H, W = c.h * c.s, c.w * c.s
            o = {"c": seeded(n + ".c", c.NH, c.B, c.Dl, c.h, c.w), "m5": seeded(n + ".m5", c.B, 5, H, W), "mt3": seeded(n + ".mt3", c.B, 3, H, W),
                 "G": seeded(n + ".G", c.NH, c.B, H, W)}
        else:
            o = {"c": seeded(n + ".c", c.NH, c.B, c.Dl, c.h, c.w), "G": seeded(n + ".G", c.NH, c.B, c.H, c.W)}
        ref, got = evaluate(c, o, torch.float64, "cpu", False), evaluate(c, o, torch.float64, "cpu", True)
        for k in ref:
            gaps[f"{type(c).__name__}{tuple(c[:6])}.{k}"] = float((got[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-300)
    return gaps


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_class():
    assert missing_classes() == []


@pytest.mark.parametrize("name", sorted(CASES))
def test_context_fp64(ecm, name):
    """Every output and gradient of one case of the table: the fp64 bound, exact structure, bit-identical repeats."""
    run_case(ecm, name)
