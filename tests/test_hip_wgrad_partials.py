"""The fixed-order sum of the weight gradients' partials (csrc/partial_sum.h, `ecm_sum_partials`) at every remainder of its loop:
eight lane groups each take every eighth partial, four at a time (a body of 32 partials) and then one at a time, so partial counts
of 1, 7, 8, 9, 31, 32 and 33 leave groups empty, put exactly one partial in each, start the second round, stop one short of the
unrolled body, fill it exactly and spill one partial into the remainder loop.

Reached through the direct 3x3x3 weight gradient (ops._wgrad_direct, ecm_conv3d_k3_wgrad), whose partial count is its worker count
P; with 8 -> 8 channels the cap is 256 workers, so P is the tile count, and batch and extents are chosen to give it -- asserted from
the restated plan (tests/test_wgrad_plan_cpu.py), not assumed.  Yardstick: the one of tests/test_hip_conv3d_fp64.py, imported (its
K and FLOOR, its fp64 reference and its fp32 draws); two runs must agree bit for bit."""
import pytest
import torch

import test_hip_conv3d_fp64 as T
import test_wgrad_plan_cpu as WP

pytestmark = pytest.mark.gpu

# P -> (B, (D, H, W)): tiles of 2 x 8 x 16 output voxels at stride 1
SHAPES = {1: (1, (2, 7, 13)), 7: (7, (2, 8, 16)), 8: (2, (2, 16, 32)), 9: (1, (6, 24, 16)), 31: (31, (1, 5, 9)), 32: (4, (4, 16, 32)),
          33: (3, (2, 88, 16))}


@pytest.fixture(scope="module")
def ecm():
    assert torch.cuda.is_available()
    import ecm_amd
    return ecm_amd


@pytest.mark.parametrize("P", sorted(SHAPES))
def test_direct_wgrad_at_partial_count(ecm, P):
    B, dims = SHAPES[P]
    c = T.Case("wgrad", B, 8, 8, dims, 1, False)
    ntiles, workers, _ = WP.plan_3d(B, c.Ci, c.Co, *dims, 1)
    assert ntiles == workers == P, "the shape no longer gives this partial count"
    x, w, G, Gs = T._operands("partials.%d" % P, c)
    runs = [ecm.ops._wgrad_direct(x.to(T.DEV), G.to(T.DEV), c.Co, c.Ci, 1) for _ in range(2)]
    q64 = T._torch(c, x, w, G, Gs, torch.float64, "cpu")["gw"]
    e32 = max(float((T._torch(c, x, w, G, Gs, torch.float32, dev)["gw"].cpu().double() - q64).abs().max()) for dev in ("cpu", T.DEV))
    err, scale = float((runs[0].cpu().double() - q64).abs().max()), float(q64.abs().max())
    bound = T.K * e32 + T.FLOOR * scale
    print(f"WGPARTIALS P={P} ratio {err / bound:.3f}   # err {err:.3e}, e32 {e32:.3e}, max|ref| {scale:.3e}")
    ecm.ops.check_async_errors()
    assert runs[0].shape == q64.shape and err <= bound, f"P={P}: |hip - fp64| = {err:.3e} > {T.K} * {e32:.3e} + {T.FLOOR} * {scale:.3e}"
    assert torch.equal(runs[0], runs[1]), f"P={P}: two runs differ in {int((runs[0] != runs[1]).sum())} elements"
