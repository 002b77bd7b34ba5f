"""CPU: tests/cls_batch_ref.py -- the numpy restatement wsc_cls_train_batch is held against -- equals, BIT FOR BIT, the chain Keras'
generator runs on a sample: PIL Image.resize(NEAREST) -> np.float32 -> scipy.ndimage.affine_transform(order=1) per channel ->
[::-1] flips -> the fp32 standardisation written with numpy.  No tolerance and no excused case: target sizes (1, 1), (3, 5),
(8, 8), (17, 33), sources (1, 1), (5, 23), (16, 16), (40, 31) and the target itself, the modes nearest / reflect / constant, cval
0 and 37.5, the fixed transforms of cls_batch_ref.named_affines (a shift of 2.5 image widths among them: more than one reflection
period) and the VOC2012 generator's draw ranges at 50 seeds.  Then facts that can be checked by hand."""
import numpy as np
import pytest
from PIL import Image
from scipy import ndimage

from tests import cls_batch_ref as ref
from wsscam import cls_train

MODES = ("nearest", "reflect", "constant")


def oracle_sample(img, hw, affine, flags, mode, cval, sub3, div, mul):
    """the chain itself, on PIL and scipy"""
    H, W = hw
    if img.shape[:2] != (H, W):
        img = np.asarray(Image.fromarray(img).resize((W, H), Image.NEAREST))
    x = np.asarray(img, dtype=np.float32)
    if flags & ref.FLAG_WARP:
        m, off = np.array([[affine[0], affine[1]], [affine[2], affine[3]]], np.float64), np.array([affine[4], affine[5]], np.float64)
        x = np.stack([ndimage.affine_transform(x[:, :, c], m, off, order=1, mode=mode, cval=cval) for c in range(3)], axis=2)
        assert x.dtype == np.float32
    if flags & ref.FLAG_FLIP_COLS:
        x = x[:, ::-1]
    if flags & ref.FLAG_FLIP_ROWS:
        x = x[::-1]
    x = np.array(x, np.float32, copy=True)
    for c in range(3):
        x[:, :, c] -= np.float32(sub3[c])
    x = x / np.float32(div)
    x *= np.float32(mul)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist(), got[diff][0], want[diff][0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", ref.TARGETS)
def test_fixed_transforms_equal_pil_and_scipy(hw, mode):
    n = 0
    for name, affine in ref.named_affines(*hw).items():
        for s, src in enumerate(ref.sources_for(hw)):
            img = ref.image(100 + s, src)
            for k, cval in enumerate(ref.CVALS):
                flags = ref.FLAG_WARP | (((n + k) % 4) << 1)  # none, columns, rows, both
                sub3, div, mul = ref.STANDARDISE[("ADP", "VOC2012", "DeepGlobe")[n % 3]]
                want = oracle_sample(img, hw, affine, flags, mode, cval, sub3, div, mul)
                _same_bits(ref.sample(img, hw, affine, flags, mode, cval, sub3, div, mul), want, (name, src, cval, flags))
                n += 1
    assert n == 8 * 5 * 2


@pytest.mark.parametrize("mode", MODES)
def test_voc_draw_ranges_at_50_seeds(mode):
    sub3, div, mul = ref.STANDARDISE["VOC2012"]
    warped = 0
    for seed in range(50):
        hw = ref.TARGETS[1:][seed % 3]
        srcs = ref.sources_for(hw)
        affine, flags = ref.voc_draws(seed, hw[0], hw[1], 2)
        for k in range(2):
            img = ref.image(seed, srcs[(seed + k) % len(srcs)])
            want = oracle_sample(img, hw, affine[k], int(flags[k]), mode, ref.CVALS[seed % 2], sub3, div, mul)
            _same_bits(ref.sample(img, hw, affine[k], int(flags[k]), mode, ref.CVALS[seed % 2], sub3, div, mul), want, (seed, k))
            warped += int(flags[k]) & 1
    assert warped == 100  # every VOC draw rotates, shifts and zooms


@pytest.mark.parametrize("hw", ref.TARGETS)
def test_without_the_warp_flag_the_chain_is_resize_flip_standardise(hw):
    for s, src in enumerate(ref.sources_for(hw)):
        img = ref.image(7 + s, src)
        for flags in (0, ref.FLAG_FLIP_COLS, ref.FLAG_FLIP_ROWS, ref.FLAG_FLIP_COLS | ref.FLAG_FLIP_ROWS):
            for name in ("ADP", "VOC2012", "DeepGlobe"):
                want = oracle_sample(img, hw, None, flags, "nearest", 0.0, *ref.STANDARDISE[name])
                _same_bits(ref.sample(img, hw, None, flags, "nearest", 0.0, *ref.STANDARDISE[name]), want, (src, flags, name))


def test_the_far_shift_leaves_the_first_reflection_period():
    """the case the fixed list exists for: every coordinate of the 2.5-width shift lies beyond -2 W"""
    H, W = 17, 33
    a = ref.named_affines(H, W)["shift-2.5-widths"]
    cols = a[5] + np.arange(W) * a[3]
    assert (np.abs(cols) > 2 * W).all()


# ---- facts that can be checked by hand ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_identity_warp_returns_the_input(mode):
    plane = ref.image(3, (5, 23))[:, :, 0].astype(np.float32)
    assert np.array_equal(ref.warp_plane(plane, ref.IDENTITY, mode, 37.5), plane)


def test_integer_shift_under_constant_moves_pixels_and_fills_with_cval():
    plane = ref.image(4, (8, 8))[:, :, 1].astype(np.float32)
    got = ref.warp_plane(plane, (1.0, 0.0, 0.0, 1.0, 2.0, -3.0), "constant", 37.5)  # out[r][c] = in[r + 2][c - 3]
    want = np.full((8, 8), np.float32(37.5))
    want[0:6, 3:8] = plane[2:8, 0:5]
    assert np.array_equal(got, want)


def test_all_ranges_zero_give_no_matrix():
    aug = cls_train.ImageAugmenter()
    rng = np.random.RandomState(0)
    for _ in range(5):
        p = aug.get_random_transform((17, 33, 3), rng)
        assert aug.transform_matrix(p, 17, 33) is None and aug.affine(p, 17, 33) == (None, 0)
    flips = cls_train.ImageAugmenter(horizontal_flip=True, vertical_flip=True)
    seen = {flips.affine(flips.get_random_transform((17, 33, 3), rng), 17, 33) for _ in range(64)}
    assert seen == {(None, 0), (None, 2), (None, 4), (None, 6)}


def test_presets_standardise_a_known_pixel():
    """the pixel (200, 100, 50): ADP (v - 193.09203) / 56.4501381, VOC2012 (v - (104, 117, 123)) / 255, DeepGlobe v / 255"""
    img = np.array([[[200, 100, 50]]], np.uint8)
    hand = {"ADP": (0.12237295, -1.64910192, -2.53483936), "VOC2012": (0.37647059, -0.06666667, -0.28627451),
            "DeepGlobe": (0.78431373, 0.39215686, 0.19607843)}
    for name, values in hand.items():
        for train in (False, True):
            sub3, div, mul = cls_train.ImageAugmenter.for_dataset(name, train).standardisation()
            assert (tuple(np.float32(s) for s in sub3), np.float32(div), np.float32(mul)) == (
                tuple(np.float32(s) for s in ref.STANDARDISE[name][0]), ref.STANDARDISE[name][1], ref.STANDARDISE[name][2])
            got = ref.sample(img, (1, 1), None, 0, "nearest", 0.0, sub3, div, mul).reshape(3)
            # the hand values are exact quotients; float32 adds: the constant 193.09203 rounded (<= 7.7e-6, / 56.45 = 1.4e-7)
            # and three roundings of a value below 4 (<= 2.4e-7 / 2 each): 5e-7 in all
            assert np.abs(got.astype(np.float64) - np.array(values)).max() < 5e-7, (name, got)
            v = np.array([200, 100, 50], np.float32)
            assert np.array_equal(got, ((v - np.asarray(sub3, np.float32)) / np.float32(div)) * np.float32(mul))
    assert ref.STANDARDISE["ADP"][1] == np.float32(56.450138 + 1e-7) and ref.STANDARDISE["VOC2012"][2] == np.float32(1 / 255)


def test_presets_are_the_generators_of_02_cues():
    voc = cls_train.ImageAugmenter.for_dataset("VOC2012", True)
    assert (voc.rotation_range, voc.width_shift_range, voc.height_shift_range, voc.zoom_range, voc.fill_mode, voc.horizontal_flip,
            voc.vertical_flip) == (30, 0.1, 0.1, [0.8, 1.2], "reflect", True, False)
    non = cls_train.ImageAugmenter.for_dataset("VOC2012", False)
    assert (non.rotation_range, non.zoom_range, non.horizontal_flip, non.fill_mode) == (0, [1, 1], False, "nearest")
    adp = cls_train.ImageAugmenter.for_dataset("ADP", True)
    assert (adp.horizontal_flip, adp.vertical_flip, adp.rotation_range, adp.rescale) == (True, True, 0, None)
    dg = cls_train.ImageAugmenter.for_dataset("DeepGlobe_train75", True)
    assert (dg.horizontal_flip, dg.vertical_flip, dg.preprocessing) == (True, True, None)
    for bad in ({"channel_shift_range": 10.0}, {"brightness_range": (0.5, 1.5)}, {"featurewise_center": True}, {"zca_whitening": True},
                {"samplewise_std_normalization": True}, {"fill_mode": "wrap"}, {"width_shift_range": 3}):
        with pytest.raises(ValueError):
            cls_train.ImageAugmenter(**bad)


def test_draws_come_from_the_callers_generator_in_keras_order():
    """theta, tx (times the height), ty (times the width), (zx, zy) as one uniform(size=2), two coins -- and the global generator
    is not touched"""
    aug = cls_train.ImageAugmenter.for_dataset("VOC2012", True)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    p = aug.get_random_transform((17, 33, 3), np.random.RandomState(11))
    assert np.array_equal(np.random.get_state()[1], before)
    r = np.random.RandomState(11)
    theta, tx, ty = r.uniform(-30, 30), r.uniform(-0.1, 0.1) * 17, r.uniform(-0.1, 0.1) * 33
    zx, zy = r.uniform(0.8, 1.2, 2)
    fh, fv = r.random_sample() < 0.5, r.random_sample() < 0.5
    assert (p["theta"], p["tx"], p["ty"], p["shear"], p["zx"], p["zy"], p["flip_horizontal"], p["flip_vertical"]) == (
        theta, tx, ty, 0, zx, zy, bool(fh), False)
    with pytest.raises(TypeError):
        aug.get_random_transform((17, 33, 3), np.random)
