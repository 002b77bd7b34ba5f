"""CPU: the float64 layer references of tests/layer_ref.py against torch.nn modules and hand-written loops on the same data."""
import numpy as np
import pytest
import torch

from tests import helpers, layer_ref as lr
from wsscam import _lib


def _values(rng, n):
    """both signs, magnitudes from half's subnormals to its upper range"""
    return (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-7, 3, n)).astype(np.float32)


def test_as_precision_one_plane_and_f32():
    x = _values(np.random.default_rng(0), 4096)
    assert np.array_equal(lr.as_precision(x, _lib.PREC_BF16), helpers.bf16_round(x))
    assert np.array_equal(lr.as_precision(x, _lib.PREC_F16), helpers.f16_round(x))
    assert np.array_equal(lr.as_precision(x, _lib.PREC_F32), x)
    assert lr.as_precision(x, _lib.PREC_F32) is not x


@pytest.mark.parametrize("prec", lr.TWO_PLANE, ids=lambda p: lr.PREC_NAME[p])
def test_as_precision_two_planes_sum_exactly(prec):
    x = _values(np.random.default_rng(1), 4096)
    rnd = helpers.bf16_round if prec == _lib.PREC_BF16X3 else helpers.f16_round
    hi, lo = lr.planes(x, prec)
    assert np.array_equal(hi, rnd(x)) and np.array_equal(lo, rnd(x - hi))
    v = lr.as_precision(x, prec)
    # the fp32 sum of the planes IS their exact sum, and the value is a fixed point: staging it again changes nothing
    assert np.array_equal(v.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))
    assert np.array_equal(lr.as_precision(v, prec), v)
    # two planes hold x to the mode's half-ulp (IEEE half: plus half a subnormal spacing)
    assert (np.abs(v.astype(np.float64) - x) <= lr.HALF_ULP[prec] * np.abs(x) + lr.ABS_FLOOR[prec]).all()


def test_group_norm_head_matches_torch_module():
    rng = np.random.default_rng(2)
    N, H, W, C, G, Ctot, coff = 2, 5, 7, 12, 3, 20, 4
    x = (rng.normal(0, 2, (N, H, W, C)) + rng.normal(0, 3, C)).astype(np.float32)
    gamma, beta = rng.normal(0, 1, C), rng.normal(0, 1, C)
    gamma[1] = 0.0
    gn = torch.nn.GroupNorm(G, C, eps=1e-5).double()
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(gamma))
        gn.bias.copy_(torch.from_numpy(beta))
        want = gn(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    y0 = rng.normal(0, 1, (N, H, W, Ctot))
    for relu in (0, 1):
        got = lr.group_norm_head(x, gamma, beta, G, 1e-5, 1, relu, H, W, y0, coff)
        w = np.maximum(want, 0) if relu else want
        assert np.abs(got[..., coff:coff + C] - w).max() < 1e-12
        assert np.array_equal(got[..., :coff], y0[..., :coff]) and np.array_equal(got[..., coff + C:], y0[..., coff + C:])
    # the statistics the bound of the device test is built from are this normalisation's
    mean, rstd, amax = lr.group_stats(x, G, 1e-5)
    Cg = C // G
    manual = (x.astype(np.float64) - np.repeat(mean, Cg, 1)[:, None, None, :]) * np.repeat(rstd, Cg, 1)[:, None, None, :] * gamma + beta
    assert np.abs(manual - want).max() < 1e-12
    assert amax.shape == (N, G) and np.isclose(amax.max(), np.abs(x).max())


def test_group_norm_head_upsample_commutes_and_crops():
    """GroupNorm is a per-channel affine map and the bilinear weights sum to 1: interpolating x first and normalising with the
    statistics of the SOURCE map (the kernel's order) is the reference's normalise-then-interpolate."""
    rng = np.random.default_rng(3)
    N, H, W, C, G, up, Hd, Wd = 2, 3, 5, 8, 2, 2, 5, 9
    x = rng.normal(0, 1, (N, H, W, C)).astype(np.float32)
    gamma, beta = rng.normal(0, 1, C), rng.normal(0, 1, C)
    got = lr.group_norm_head(x, gamma, beta, G, 1e-5, up, 0, Hd, Wd, np.zeros((N, Hd, Wd, C)), 0)
    mean, rstd, _ = lr.group_stats(x, G, 1e-5)
    xi = torch.nn.functional.interpolate(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), scale_factor=up, mode="bilinear",
                                         align_corners=False).permute(0, 2, 3, 1).numpy()[:, :Hd, :Wd]
    Cg = C // G
    other = (xi - np.repeat(mean, Cg, 1)[:, None, None, :]) * np.repeat(rstd, Cg, 1)[:, None, None, :] * gamma + beta
    assert got.shape == (N, Hd, Wd, C) and np.abs(got - other).max() < 1e-12


@pytest.mark.parametrize("geom", [(3, 2, 1), (2, 2, 0)], ids=lambda g: "k%ds%dp%d" % g)
def test_max_pool_against_window_loop(geom):
    k, stride, pad = geom
    rng = np.random.default_rng(4)
    x = rng.normal(-1, 2, (2, 5, 5, 3)).astype(np.float32)
    x[0, :, :, 0] = -np.abs(x[0, :, :, 0]) - 0.25  # a plane of negatives: padding must not win
    Ho = (5 + 2 * pad - k) // stride + 1
    want = np.empty((2, Ho, Ho, 3))
    for n in range(2):
        for c in range(3):
            for ho in range(Ho):
                for wo in range(Ho):
                    taps = [x[n, hi, wi, c] for hi in range(ho * stride - pad, ho * stride - pad + k) if 0 <= hi < 5
                            for wi in range(wo * stride - pad, wo * stride - pad + k) if 0 <= wi < 5]
                    want[n, ho, wo, c] = max(taps)
    got = lr.max_pool(x, k, stride, pad)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert (got[0, :, :, 0] < 0).all()


def test_small_references_on_hand_values():
    head = np.array([[[[1.0, -2.0], [3.0, 4.0]]], [[[-5.0, 6.0], [7.0, -8.0]]]], np.float32)  # (2, 1, 2, 2): B = 1, h = 1, w = 2
    cam = lr.flip_add(head, 2)
    assert cam.shape == (1, 2, 1, 2)
    assert np.array_equal(cam[0, :, 0, :], np.array([[1.0 + 7.0, 3.0 + 0.0], [0.0 + 0.0, 4.0 + 6.0]], np.float32))
    e = np.arange(2 * 2 * 3, dtype=np.float32).reshape(2, 2, 3)
    d = np.arange(2 * 2 * 3 * 2, dtype=np.float32).reshape(2, 2, 3, 2)
    edge, dp = lr.edge_finish(e, d, 1, 2, (0.5, -1.0))
    z = np.array([[0.0 / 2 + 7.0 / 2, 1.0 / 2 + 6.0 / 2]])  # row 0 of e[1] cropped to 2 columns is (6, 7), flipped (7, 6)
    assert np.allclose(edge[0], 1 / (1 + np.exp(-z)), rtol=0, atol=1e-15)
    assert np.array_equal(dp[0, :, 0, :], np.array([[0 - 0.5, 2 - 0.5], [1 + 1.0, 3 + 1.0]], np.float32))
    feat = np.array([[[1.0, 2.0], [3.0, -4.0]], [[9.0, 9.0], [9.0, 9.0]]], np.float32)  # 2 samples, 2 positions, F = 2
    s, g = lr.gap_linear_sigmoid(feat, np.array([[1.0, -1.0]]), np.array([0.5]), False, 2)
    assert np.array_equal(g, [[2.0, -1.0]]) and np.allclose(s, 1 / (1 + np.exp(-3.5)))
    s, g = lr.gap_linear_sigmoid(feat, np.array([[1.0, -1.0]]), None, True, 1)
    assert np.array_equal(g, [[3.0, 2.0], [9.0, 9.0]]) and np.allclose(s[:, 0], [1 / (1 + np.exp(-1.0)), 0.5])
