"""Host: tests/seg_sgd_ref.py, the numpy statement of the optimiser step the GPU tests compare bits with, held to facts that can be
checked by hand."""
import numpy as np
import pytest

from tests import deeplab_ref as ref
from tests import seg_sgd_ref as sgd

U = 2.0 ** -24


def _case(method, C, seed=0):
    weights = ref.random_weights(method, C, 64, 128, seed=seed)
    layout, n = sgd.layout_of(method, weights)
    return weights, layout, n, sgd.segments(layout)


def test_layout_has_no_gaps_and_odd_offsets():
    _, layout, n, segs = _case("DSRG", 5)
    assert segs[0][1] == 0 and segs[-1][2] == n
    assert all(a[2] == b[1] for a, b in zip(segs[:-1], segs[1:]))  # no gaps, in offset order
    assert [s[0] for s in segs[:2]] == ["conv1_1.w", "conv1_1.b"] and layout["conv1_1"]["Cin"] == 3
    assert layout["fc6_2"]["w_off"] % 2 == 1  # behind fc8_1's five biases every offset is odd


def test_constant_gradient_closed_form():
    """constant g, wd = 0, accum_num = 1: param_n = param_0 - lr g sum_{k=1..n} (1 - m^k) / (1 - m) in the float64 twin"""
    _, _, n, segs = _case("SEC", 5)
    ones = [(name, a, b, 1.0, decay) for name, a, b, _, decay in segs]  # (the multipliers have a test of their own)
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(n)
    g = rng.standard_normal(n)
    lr, m, steps = 1e-2, 0.9, 7
    p, acc, mom = p0.copy(), np.zeros(n), np.zeros(n)
    for _ in range(steps):
        acc = sgd.accumulate(ones, p, g, acc, 0.0, 1, np.float64)
        p, acc, mom = sgd.apply(p, acc, mom, lr, m, True, np.float64)
    want = p0 - lr * g * sum((1 - m ** k) / (1 - m) for k in range(1, steps + 1))
    assert np.abs(p - want).max() <= 1e-13 * np.abs(want).max()
    assert not acc.any()


@pytest.mark.parametrize("method", ["SEC", "DSRG"])
@pytest.mark.parametrize("C", [5, 21])
def test_multipliers_by_segment(method, C):
    weights, layout, n, segs = _case(method, C)
    acc = sgd.accumulate(segs, sgd.flatten(layout, n, weights), np.ones(n, np.float32), np.zeros(n, np.float32), 0.0, 1)
    got = sgd.unflatten(layout, acc)
    for layer in ref.layer_names(method):
        fc8 = layer.startswith("fc8")
        assert (got[layer]["w"] == (10.0 if fc8 else 1.0)).all() and (got[layer]["b"] == (20.0 if fc8 else 2.0)).all(), layer
    assert sum(l.startswith("fc8") for l in layout) == (1 if method == "SEC" else 4)


def test_decay_touches_weights_only():
    weights, layout, n, segs = _case("DSRG", 5)
    p = sgd.flatten(layout, n, weights)
    zero = np.zeros(n, np.float32)
    got = sgd.unflatten(layout, sgd.accumulate(segs, p, zero, zero, 0.5, 1))
    for layer in layout:
        mult = 10.0 if layer.startswith("fc8") else 1.0
        assert np.array_equal(got[layer]["w"], np.float32(mult) * (np.float32(0.5) * weights[layer]["w"])), layer
        assert not got[layer]["b"].any() and np.abs(weights[layer]["b"]).max() > 0
    want_l2 = sum(0.5 * float((weights[l]["w"].astype(np.float64) ** 2).sum()) for l in layout)
    assert abs(sgd.l2(segs, p) - want_l2) <= 1e-12 * want_l2


def test_float32_within_seven_roundings_of_float64():
    """every float32 operation is one rounding (2^-24 relative) away from the float64 twin's on the same operands: accumulate
    (wd *, +, mult *, /, +) and apply (*, +; lr *, -) change param by at most 8 x 2^-24 max(|param|, lr |mom|) -- 7 roundings
    reach it, rounded up -- and mom, accum by at most 8 x 2^-24 of the sum of the magnitudes of their terms"""
    _, _, n, segs = _case("DSRG", 21)
    rng = np.random.default_rng(2)
    p, g, a, m = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    wd, lr, mo = (float(np.float32(v)) for v in (5e-4, 1e-4, 0.9))  # the constants as float32 holds them, for both
    acc32 = sgd.accumulate(segs, p, g, a, wd, 3)
    p32, _, m32 = sgd.apply(p, acc32, m, lr, mo, False)
    acc64 = sgd.accumulate(segs, p, g, a, wd, 3, np.float64)
    p64, _, m64 = sgd.apply(p, acc64, m, lr, mo, False, np.float64)
    assert acc32.dtype == p32.dtype == m32.dtype == np.float32 and p64.dtype == np.float64
    mags = sgd.accumulate(segs, np.abs(p), np.abs(g), np.abs(a), wd, 3, np.float64)  # |a| + mult (|g| + wd |p|) / n
    mag_m = np.abs(m).astype(np.float64) * mo + mags
    scale = np.maximum(np.abs(p64), lr * np.abs(m64))
    figs = (np.abs(p32 - p64) / scale).max() / U, (np.abs(acc32 - acc64) / mags).max() / U, (np.abs(m32 - m64) / mag_m).max() / U
    print("float32 against float64, in units of 2^-24: param %.3f, accum %.3f, mom %.3f" % figs)
    assert max(figs) <= 8.0


def test_three_accumulations_then_one_apply():
    _, _, n, segs = _case("SEC", 21)
    rng = np.random.default_rng(3)
    p = rng.standard_normal(n).astype(np.float32)
    gs = [(1e-3 * rng.standard_normal(n)).astype(np.float32) for _ in range(3)]
    acc = np.zeros(n, np.float32)
    for g in gs:
        acc = sgd.accumulate(segs, p, g, acc, 5e-4, 3)
    third = np.float32(3)
    by_hand = np.zeros(n, np.float32)
    for g in gs:
        for _, a, b, mult, decay in segs:
            t = g[a:b] + np.float32(5e-4) * p[a:b] if decay else g[a:b]
            by_hand[a:b] = by_hand[a:b] + (np.float32(mult) * t) / third
    assert np.array_equal(acc.view(np.uint32), by_hand.view(np.uint32))
    p1, acc1, m1 = sgd.apply(p, acc, np.zeros(n, np.float32), 1e-4, 0.9)
    assert np.array_equal(m1, acc) and np.array_equal(p1, p - np.float32(1e-4) * acc) and not acc1.any()
    # equal gradients: the accumulator is the mean up to the roundings of g / 3 summed three times
    same = np.zeros(n, np.float32)
    for _ in range(3):
        same = sgd.accumulate(segs, p, gs[0], same, 0.0, 3)
    one = sgd.accumulate(segs, p, gs[0], np.zeros(n, np.float32), 0.0, 1)
    assert np.abs(same - one).max() <= 4 * U * np.abs(one).max()


def test_lr_schedule():
    for epoch, power in ((0, 0), (3.99, 0), (4, 1), (8.5, 2)):
        assert sgd.lr_at(epoch) == np.float32(1e-4 * 0.5 ** power)
    assert sgd.lr_at(4).dtype == np.float32
