"""tests/seg_chain_ref.py (the float64 oracle of csrc/seg_chain.hip) on facts that can be checked by hand."""
import numpy as np
import pytest

from tests import seg_chain_ref as ref

MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)


@pytest.mark.parametrize("C", [1, 5, 21])
def test_uniform_marginals_give_log_one_over_c(C):
    out = ref.crf_logprob(np.full((2, C, 6), 1.0 / C), 1e-4)
    assert out.shape == (2, 6, C)
    assert np.allclose(out, np.log(1.0 / C), rtol=0, atol=1e-15)


@pytest.mark.parametrize("C", [2, 5, 21])
def test_one_hot_marginals(C):
    mp = np.float64(np.float32(1e-4))  # the kernel's min_prob is a float32
    q = np.zeros((1, C, 3))
    q[0, 1, :] = 1.0
    out = ref.crf_logprob(q, 1e-4)
    s = 1.0 + (C - 1) * mp
    want = np.full((1, 3, C), np.log(mp / s))
    want[0, :, 1] = np.log(1.0 / s)
    assert np.allclose(out, want, rtol=0, atol=1e-13)
    assert np.allclose(np.exp(out).sum(-1), 1.0, rtol=0, atol=1e-13)


def test_values_below_min_prob_are_clamped_not_dropped():
    q = np.array([[[0.5], [5e-5], [0.0], [0.49995]]])
    out = ref.crf_logprob(q, 1e-4)
    assert out[0, 0, 1] == out[0, 0, 2]  # both sit at min_prob
    assert out[0, 0, 1] > np.log(5e-5)


def test_astype_u8_rule():
    got = ref.astype_u8([-1.5, 256.7, -1e-5, 254.99, 0.0, 255.0, 255.999, 1000.25, -256.0, -257.5])
    assert got.dtype == np.uint8
    assert got.tolist() == [255, 0, 0, 254, 0, 255, 255, 232, 0, 255]
    # ... and numpy's own cast wherever the value is in range
    v = np.linspace(0.0, 255.99, 1001)
    assert np.array_equal(ref.astype_u8(v), v.astype(np.uint8))


def test_identity_size_preprocess_is_exact():
    img = np.random.default_rng(0).integers(0, 256, (11, 7, 3), dtype=np.uint8)
    got = ref.preprocess(img, MEAN, (11, 7))
    assert np.array_equal(got, img[:, :, ::-1].astype(np.float64) - MEAN.astype(np.float64))
    # the float32 form of the same thing is what the device holds
    assert np.array_equal(got.astype(np.float32), img[:, :, ::-1].astype(np.float32) - MEAN)


def test_preprocess_of_a_constant_image_is_that_constant():
    img = np.full((9, 13, 3), 0, np.uint8)
    img[:, :, 0], img[:, :, 1], img[:, :, 2] = 10, 20, 30  # R, G, B
    got = ref.preprocess(img, MEAN, (17, 5))
    assert got.shape == (17, 5, 3)
    assert np.allclose(got, np.array([30.0, 20.0, 10.0]) - MEAN.astype(np.float64), rtol=0, atol=1e-12)


def test_crf_image_identity_size_and_channel_order():
    x = np.random.default_rng(1).uniform(-120, 130, (2, 6, 5, 3)).astype(np.float32)
    got = ref.crf_image(x, MEAN, (6, 5))
    assert got.shape == (2, 6, 5, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ref.astype_u8(x + MEAN.reshape(1, 1, 1, 3)))  # no channel flip, the fp32 sum
    assert ref.crf_image(x, MEAN, (3, 2)).shape == (2, 3, 2, 3)
