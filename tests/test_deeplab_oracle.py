"""CPU: the float64 oracle of the SEC / DSRG forward pass (tests/deeplab_ref.py) against hand-checkable facts."""
import numpy as np
import pytest
import torch

from tests import deeplab_ref as ref


def test_same_output_sizes_and_pad_split():
    n, sizes = 321, []
    for _ in range(3):
        n = ref.same_pad(n, 2)[0]
        sizes.append(n)
    assert sizes == [161, 81, 41]
    assert ref.same_pad(64, 2)[0] == 32
    assert ref.same_pad(321, 2)[1:] == (1, 1) and ref.same_pad(161, 2)[1:] == (1, 1) and ref.same_pad(81, 2)[1:] == (1, 1)
    assert ref.same_pad(64, 2)[1:] == (0, 1)  # even size at stride 2: nothing before, one after
    assert ref.same_pad(41, 1) == (41, 1, 1) and ref.same_pad(1, 1) == (1, 1, 1)
    x = np.random.default_rng(0).normal(size=(1, 321, 64, 8))
    assert ref.max_pool_same(x, 2).shape == (1, 161, 32, 8)


def test_max_pool_pad_split_on_an_even_size():
    """0 / 1: output o covers inputs 2o .. 2o + 2, so the LAST column only ever competes with its left neighbours."""
    x = -np.arange(1, 9, dtype=np.float64).reshape(1, 1, 8, 1) * np.ones((1, 1, 1, 8))  # decreasing and NEGATIVE along W
    y = ref.max_pool_same(x, 2)
    assert y.shape == (1, 1, 4, 8)
    assert np.array_equal(y[0, 0, :, 0], [-1, -3, -5, -7])  # a 1 / 0 split would give -1, -2, -4, -6; zero padding would give 0
    assert ref.max_pool_same(x, 1).max() < 0  # padding never wins


def test_avg_pool_divisor_on_a_constant_map():
    y = ref.avg_pool_same(np.full((1, 5, 6, 3), 7.0))
    assert np.array_equal(y, np.full((1, 5, 6, 3), 7.0))  # 4 at a corner, 6 on an edge, 9 inside: a constant stays the constant
    ones = np.ones((1, 5, 6, 1))
    t = torch.as_tensor(ones).permute(0, 3, 1, 2)
    cnt = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(t, (1, 1, 1, 1)), 3, 1) * 9
    assert cnt[0, 0, 0, 0].round() == 4 and cnt[0, 0, 0, 2].round() == 6 and cnt[0, 0, 2, 2].round() == 9
    x = np.arange(30, dtype=np.float64).reshape(1, 5, 6, 1)
    assert ref.avg_pool_same(x)[0, 0, 0, 0] == (0 + 1 + 6 + 7) / 4 and ref.avg_pool_same(x)[0, 0, 1, 0] == (0 + 1 + 2 + 6 + 7 + 8) / 6


@pytest.mark.parametrize("hw,dil", [((9, 9), 12), ((7, 5), 7)])
def test_dilated_conv_beyond_the_map_is_its_centre_tap(hw, dil):
    rng = np.random.default_rng(3)
    x = rng.normal(size=(2,) + hw + (4,))
    w = rng.normal(size=(3, 3, 4, 6))
    b = rng.normal(size=6)
    t = torch.as_tensor(x).permute(0, 3, 1, 2)
    full = ref.conv_t(t, w, b, dil=dil, relu=False)
    centre = ref.conv_t(t, w[1:2, 1:2], b, dil=1, relu=False)
    assert full.shape == centre.shape and torch.allclose(full, centre, rtol=0, atol=1e-12)


def test_tf_resize_reproduces_source_pixels_at_multiples_of_the_factor():
    x = np.random.default_rng(4).normal(size=(2, 5, 7, 3))
    y = ref.resize_bilinear_tf(x, 20, 21)  # factors 4 and 3
    assert y.shape == (2, 20, 21, 3)
    assert np.array_equal(y[:, ::4, ::3], x)
    # between two source pixels: the plain lerp, no half-pixel offset; past the last one: clamped
    assert np.allclose(y[:, 2, 0], (x[:, 0, 0] + x[:, 1, 0]) / 2, rtol=0, atol=1e-12)
    assert np.allclose(y[:, 19, 20], x[:, 4, 6], rtol=0, atol=1e-12)
    assert np.array_equal(ref.resize_bilinear_tf(x, 5, 7), x)


def test_fc8_softmax_rows():
    x = np.random.default_rng(5).uniform(-30, 30, (50, 21))
    p = ref.fc8_softmax(x, 1e-4)
    assert np.allclose(p.sum(-1), 1.0, rtol=0, atol=1e-12) and p.min() >= 1e-4 / (1 + 21e-4) * (1 - 1e-12)


def test_wrong_layout_weights_raise():
    wts = ref.random_weights("DSRG", 5, 64, 128, seed=1)
    ref.layer_weights("DSRG", wts)
    bad = dict(wts)
    bad["conv2_1"] = {"w": np.transpose(wts["conv2_1"]["w"], (3, 2, 0, 1)), "b": wts["conv2_1"]["b"]}  # OIHW where HWIO belongs
    with pytest.raises(ValueError):
        ref.layer_weights("DSRG", bad)
    missing = {k: v for k, v in wts.items() if k != "fc8_3"}
    with pytest.raises(KeyError):
        ref.layer_weights("DSRG", missing)
    with pytest.raises(KeyError):
        ref.layer_weights("SEC", wts)  # ASPP names for the one-branch net


@pytest.mark.parametrize("case", ref.THIN_CASES, ids=lambda c: "%s-%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1]))
def test_oracle_float32_stays_within_the_gpu_tests_bounds(case):
    """The bounds tests/test_gpu_deeplab.py holds the device to (logits 1e-4 of the map's max, softmax 1e-4, arg-max agreement
    99.5 %) must not be tighter than the oracle's own float32-vs-float64 distance for the chosen seeds."""
    wts, x = ref.thin_case(*case)
    f64, p64 = ref.forward(case[0], wts, x)
    f32, p32 = ref.forward(case[0], wts, x, dtype=torch.float32)
    d = np.abs(f32 - f64).max() / np.abs(f64).max()
    agree = (f32.argmax(-1) == f64.argmax(-1)).mean()
    print("oracle f32 vs f64 %s: logits %.3g of max, softmax %.3g, arg-max agreement %.5f" % (case, d, np.abs(p32 - p64).max(), agree))
    assert d <= 1e-5 and np.abs(p32 - p64).max() <= 1e-5 and agree >= 0.999
    assert f64.shape == (2, -(-case[2][0] // 8), -(-case[2][1] // 8), case[1])
