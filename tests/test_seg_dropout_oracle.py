"""CPU: the oracle of the dropout sites (tests/seg_dropout_ref.py): Philox4x32-10 against the known-answer vectors of the
Random123 distribution, the properties of the keep-masks, and the mask-free chain rule at a dropped tape against plain autograd of
the forward pass with explicit mask multiplication."""
import numpy as np
import pytest
import torch

from tests import deeplab_grad_ref as gref
from tests import deeplab_ref as ref
from tests import seg_dropout_ref as dref

# Random123's kat_vectors for philox4x32 at 10 rounds: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter, key, want", KAT)
def test_philox_known_answers(counter, key, want):
    got = tuple(int(v[0]) for v in dref.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_philox_is_elementwise():
    """a vector of counters gives what the counters give one by one"""
    c0 = np.array([0, 0xffffffff, 0x243f6a88, 7], np.uint64)
    got = dref.philox4x32_10((c0, 5, 6, 7), (8, 9))
    for j, c in enumerate(c0):
        one = dref.philox4x32_10((int(c), 5, 6, 7), (8, 9))
        assert [int(v[j]) for v in got] == [int(v[0]) for v in one]


def test_uniform_is_exact_and_in_range():
    u = dref.uniform(4096, 3, 1, 0)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * np.float32(2.0 ** 24), np.rint(u.astype(np.float64) * 2.0 ** 24))  # 24-bit integers 2^-24


def test_drop_prob_zero_keeps_everything():
    assert dref.keep_mask((2, 9, 9, 128), 0.0, 5, 2, 3).all()
    x = np.array([-0.0, 1.5, np.inf], np.float32)
    d, keep = dref.dropout_f32(x, 0.0, 1, 2, 3)
    assert keep.all() and d.tobytes() == x.tobytes()


def test_seed_step_and_site_each_change_the_mask():
    base = dref.keep_mask((2, 9, 9, 128), 0.5, 5, 2, 3)
    for other in (dref.keep_mask((2, 9, 9, 128), 0.5, 6, 2, 3), dref.keep_mask((2, 9, 9, 128), 0.5, 5 + (1 << 32), 2, 3),
                  dref.keep_mask((2, 9, 9, 128), 0.5, 5, 3, 3), dref.keep_mask((2, 9, 9, 128), 0.5, 5, 2, 4)):
        frac = float((other != base).mean())
        assert 0.4 < frac < 0.6, frac  # (independent fair bits differ on half the elements; 20736 elements: sigma 0.0035)


def test_batch_one_mask_is_the_prefix_of_batch_two():
    two = dref.keep_mask((2, 9, 9, 128), 0.5, 5, 2, 3)
    one = dref.keep_mask((1, 9, 9, 128), 0.5, 5, 2, 3)
    assert np.array_equal(two[:1], one)


def test_first_offsets_the_element_index():
    whole = dref.keep_mask((4480 + 7,), 0.3, 9, 1, 2)
    assert np.array_equal(dref.keep_mask((4480,), 0.3, 9, 1, 2, first=7), whole[7:])
    # the counter's high word: elements 2^34 + 1 ... draw from blocks 2^32, 2^32 + 1, ... (c0 wraps to 0, c1 = 1)
    u = dref.uniform(3, 9, 1, 2, first=(1 << 34) + 1)
    w = dref.philox4x32_10((0, 1, 1, 2), (9, 0))
    assert [float(v) for v in u] == [float(np.float32(int(w[j][0]) >> 8) * np.float32(2.0 ** -24)) for j in (1, 2, 3)]


@pytest.mark.parametrize("n", [20736, 82944, 4480])
def test_kept_fraction_at_half(n):
    """within 4 sigma of n / 2 for fixed seeds (sigma = sqrt(n) / 2); the worst over these seeds is printed"""
    worst = 0.0
    for seed in range(20):
        kept = int(dref.keep_mask((n,), 0.5, seed, seed % 3, seed % 8).sum())
        worst = max(worst, abs(kept - n / 2) / (np.sqrt(n) / 2))
    print("kept fraction at 0.5, %d elements, 20 seeds: worst %.2f sigma" % (n, worst))
    assert worst <= 4.0


def test_value_rule():
    x = np.array([1.0, -0.0, 3.0, np.inf, 1e-45, 2.5, -7.0, 0.1], np.float32)
    d, keep = dref.dropout_f32(x, 0.3, 4, 0, 1)
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    for xi, di, ki in zip(x, d, keep):
        want = np.float32(xi * s) if ki else np.float32(0.0)
        assert di.tobytes() == want.tobytes()
    assert dref.scale_of(0.5) == np.float32(2.0)


# the thin cases the device's end-to-end test runs (tests/test_gpu_seg_dropout.py)
CHAIN_CASES = [("SEC", 5, (65, 65)), ("DSRG", 5, (65, 65)), ("DSRG", 21, (64, 48))]
# max over the layers of max|chain - autograd| / max|autograd| on a float64 tape, worst over CHAIN_CASES at drop_prob 0.5 and
# 0.3.  SEC measures exactly 0 (one branch: both sides do the same float64 operations); DSRG differs by the order in which the four
# branches' gradients into pool5a are summed, a few float64 roundings that the trunk's convolutions carry on -- and torch's float64
# convolution sums in an order of its CPU backend's choosing, so the figure is a property of the host as well: measured on two
# kinds of host, at 1 ... 16 threads, 2.00e-15 / 2.28e-15 on one and 3.48e-15 / 3.42e-15 on the other for ("DSRG", 5, (65, 65)) /
# ("DSRG", 21, (64, 48)) at 0.5 (at 0.3: 1.0 - 2.6e-15).  The constant is the worst of all of them; the existing pair without
# dropout measures ~2e-15.
CHAIN_VS_AUTOGRAD = 3.48e-15


@pytest.mark.parametrize("drop_prob", [0.5, 0.3])
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: "%s-%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1]))
def test_chain_on_float64_dropped_tape_is_autograd(case, drop_prob):
    """The mask-free chain rule (dz = g scale [T > 0] at fc6 / fc7) on a float64 tape of the dropout forward pass IS autograd of
    that forward pass with explicit mask multiplication: held to 1.5 x the measured CHAIN_VS_AUTOGRAD."""
    method, C, hw = case
    weights, x = ref.thin_case(method, C, hw)
    drop = (drop_prob, 77, 3)
    tape, fc8 = dref.forward_tape_drop(method, weights, x, drop, torch.float64)
    rng = np.random.default_rng(900 + 3 * C + hw[1] + (1 if method == "SEC" else 0))
    dfc8 = (1e-3 * rng.standard_normal(fc8.shape)).astype(np.float32)
    # the tape is dropped: about the site's share of every fc entry is exactly zero where the mask drops, and nowhere else by it
    for k, (sfx, _) in enumerate(gref.branches(method)):
        for layer in (6, 7):
            t = tape["fc%d%s" % (layer, sfx)]
            m = dref.keep_mask(t.shape, drop_prob, 77, 3, dref.site_of(k, layer))
            assert not t[~m].any() and t[m].any()
    chain = dref.chain_grads_drop(method, weights, tape, dfc8, drop_prob, torch.float64)
    auto = dref.autograd_grads_drop(method, weights, x, dfc8, drop, torch.float64)
    ratios = gref.layer_ratio(chain, auto)
    worst = max(max(r) for r in ratios.values())
    print("dropout chain on a float64 tape vs autograd, %s at %.1f: worst %.2e" % (case, drop_prob, worst))
    assert worst <= 1.5 * CHAIN_VS_AUTOGRAD
    # and it is not the gradient without dropout: fc7's differs by far more than round-off
    plain = gref.chain_grads(method, weights, tape, dfc8, torch.float64)
    sfx = gref.branches(method)[0][0]
    assert gref.layer_ratio(plain, auto)["fc7" + sfx][0] > 1e-3
