"""Host: the float64 references of tests/label_tail_ref.py pinned to something other than themselves -- torch.double's own
F.interpolate / torch.max / F.pad / torch.argmax (the four lines of make_sem_seg_labels the reference runs) and examples small
enough to check by hand."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import label_tail_ref as ref

# (K, h, w) -> up -> crop: non-square, a 1 x 1 source, the identity, up-sized then cropped, a size below the source's
RESIZE_CASES = [((3, 9, 11), (36, 44), (33, 41)), ((1, 1, 1), (5, 7), (5, 7)), ((4, 16, 16), (16, 16), (16, 16)),
                ((2, 7, 5), (30, 17), (30, 17)), ((5, 13, 6), (52, 24), (49, 21)), ((3, 50, 73), (8, 12), (8, 12)),
                ((1, 7, 6), (1, 1), (1, 1)), ((2, 1, 9), (4, 33), (3, 33))]


def _torch_up(x, up, crop):
    return F.interpolate(torch.from_numpy(x).double()[None], size=tuple(up), mode="bilinear", align_corners=False)[0, :, :crop[0], :crop[1]]


@pytest.mark.parametrize("khw,up,crop", RESIZE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_upsample_vs_torch_double(khw, up, crop):
    rng = np.random.default_rng(sum(khw) + up[0])
    x = rng.normal(0, 1, khw)
    got = ref.upsample_bilinear(x, up)[:, :crop[0], :crop[1]]
    want = _torch_up(x, up, crop).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    if up == khw[1:]:
        assert np.array_equal(got, x)  # the identity resize has weights of exactly 1 and 0


def _torch_tail(rw, up, crop, keys, has_bg, thr):
    """make_sem_seg_labels.py:73-79 in torch.double on the CPU."""
    rw_up = F.interpolate(torch.from_numpy(rw).double()[:, None], size=tuple(up), mode="bilinear", align_corners=False)[..., 0, :crop[0], :crop[1]]
    rw_up = rw_up / torch.max(rw_up)
    if has_bg:
        rw_up = F.pad(rw_up, (0, 0, 0, 0, 1, 0), value=thr)
    return np.asarray(keys)[torch.argmax(rw_up, dim=0).numpy()], rw_up.numpy()


@pytest.mark.parametrize("has_bg", [False, True])
@pytest.mark.parametrize("khw,up,crop", RESIZE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_sem_seg_finish_vs_torch_double(khw, up, crop, has_bg):
    rng = np.random.default_rng(sum(khw) + crop[1])
    rw = rng.random(khw) ** 2
    keys = list(rng.permutation(np.arange(1, 255))[: khw[0] + int(has_bg)])
    keys[-1] = 255
    lab, stack = ref.sem_seg_finish(rw, up, crop, keys, has_bg, 0.3)
    want, wstack = _torch_tail(rw, up, crop, keys, has_bg, 0.3)
    assert lab.dtype == np.uint8 and lab.shape == tuple(crop)
    assert np.abs(stack - wstack).max() <= 1e-12
    assert np.array_equal(lab, want)
    assert stack[int(has_bg):].max() == 1.0  # one maximum over every map and cropped pixel, and it divides to exactly 1


@pytest.mark.parametrize("has_bg", [False, True])
def test_sem_seg_finish_zero_image_first_nan(has_bg):
    """0 / 0 everywhere: torch.argmax (and np.argmax) return the first NaN -- channel 1 behind a background channel, else 0."""
    rw = np.zeros((3, 4, 5))
    keys = [9, 17, 3, 255] if has_bg else [17, 3, 255]
    lab, stack = ref.sem_seg_finish(rw, (8, 10), (7, 9), keys, has_bg, 0.25)
    with np.errstate(invalid="ignore"):
        want, _ = _torch_tail(rw, (8, 10), (7, 9), keys, has_bg, 0.25)
    assert np.isnan(stack[int(has_bg):]).all()
    assert np.array_equal(lab, want) and (lab == 17).all()
    assert np.isinf(ref.top_two_margin(stack)).all()


def test_sem_seg_finish_constant_map_threshold():
    """A constant map normalises to exactly 1 everywhere: background (the first maximum) at bg_thres = 1.0, foreground just below."""
    rw = np.full((1, 3, 4), 0.37)
    lab, stack = ref.sem_seg_finish(rw, (9, 12), (9, 11), [0, 15], True, 1.0)
    assert (stack[1] == 1.0).all() and (lab == 0).all()
    lab, _ = ref.sem_seg_finish(rw, (9, 12), (9, 11), [0, 15], True, np.nextafter(1.0, 0.0))
    assert (lab == 15).all()


def test_sem_seg_finish_identical_maps_first_key():
    rng = np.random.default_rng(3)
    a = rng.random((5, 6)) ** 2
    rw = np.stack([a, 0.1 * rng.random((5, 6)), a])  # map 2 is map 0's bits
    lab, stack = ref.sem_seg_finish(rw, (20, 24), (18, 24), [40, 41, 42], False, 0.0)
    assert not (lab == 42).any() and (lab == 40).any()
    lab2, _ = ref.sem_seg_finish(rw[:2], (20, 24), (18, 24), [40, 41], False, 0.0)
    assert np.array_equal(lab, lab2)
    assert (ref.top_two_margin(stack)[lab == 40] == 0).all()


def test_sem_seg_finish_maximum_is_over_the_crop():
    """The peak of the up-sized map lies in the band the crop removes: the normaliser is the cropped maximum."""
    rw = np.full((1, 2, 2), 0.25)
    rw[0, 1, 1] = 1.0
    lab, stack = ref.sem_seg_finish(rw, (8, 8), (5, 5), [0, 7], True, 0.9)
    up = ref.upsample_bilinear(rw, (8, 8))
    assert up.max() == 1.0 and up[:, :5, :5].max() < 0.7
    assert stack[1].max() == 1.0 and (lab == 7).any()  # a maximum over the whole 8 x 8 map would leave every pixel background
    assert not (up[0, :5, :5] / up.max() > 0.9).any()


def test_label_unary_from_cam_by_hand():
    t = np.float32(0.3)
    maps = np.array([[0.1, 0.3, 0.5, 0.9, 0.2],
                     [0.2, 0.3, 0.5, 0.4, np.nextafter(t, np.float32(1))]], np.float32)
    maps[:, 1] = t  # equal to the threshold: the padded channel came first
    lab, U = ref.label_unary_from_cam(maps, 0.3, 0.7)
    assert lab.dtype == np.int32 and lab.tolist() == [0, 0, 1, 1, 2]
    g = np.float64(np.float32(0.7))
    p, n = np.float32(-np.log(g)), np.float32(-np.log((1 - g) / 2))
    assert U.dtype == np.float32 and U.shape == (3, 5)
    for i, l in enumerate(lab):
        assert U[l, i] == p and (np.delete(U[:, i], l) == n).all()
    assert abs(float(p) - 0.35667) < 1e-5 and abs(float(n) - 1.89712) < 1e-5


def test_ir_label_combine_by_hand():
    """cam_to_ir_label.py:56-58 and :39-40 on a 3 x 3 example written out."""
    keys = np.array([0, 3, 15, 255])  # voc12: np.pad(cam keys + 1, (1, 0))
    fg = np.array([[0, 0, 1], [2, 3, 0], [1, 0, 2]])
    bg = np.array([[0, 1, 1], [2, 0, 0], [0, 3, 2]])
    want = np.array([[0, 255, 3], [15, 255, 0], [3, 255, 15]], np.uint8)
    # fg 0 / bg 0 -> 0 (confident background); fg 0 / bg != 0 -> 255 (unsure); fg != 0 -> its key whatever bg says
    got = ref.ir_label_combine(fg.ravel(), bg.ravel(), keys).reshape(3, 3)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # the reference's three lines, verbatim
    fg_conf, bg_conf = keys[fg], keys[bg]
    conf = fg_conf.copy()
    conf[fg_conf == 0] = 255
    conf[bg_conf + fg_conf == 0] = 0
    assert np.array_equal(conf.astype(np.uint8), want)
    # ADP / DeepGlobe: keys[0] = -1, class id 0 is a real class
    keys = np.array([-1, 0, 4])
    fg = np.array([[0, 0, 1], [2, 1, 0], [1, 0, 2]])
    want = np.array([[255, 255, 0], [4, 0, 255], [0, 255, 4]], np.uint8)
    assert np.array_equal(ref.ir_label_combine(fg.ravel(), None, keys).reshape(3, 3), want)


def test_cam_sum_scales_order():
    cam = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [3.0], [4.0], [5.0]], np.float32)
    got = ref.cam_sum_scales(cam, 3)
    assert got.dtype == np.float32 and got.tolist() == [[1.0], [12.0]]  # (1 + 2^-24) rounds back to 1, twice
    assert np.float32(np.float32(2.0 ** -24) + np.float32(2.0 ** -24)) + np.float32(1.0) != 1.0  # another order gives other bits
    assert np.array_equal(ref.cam_sum_scales(cam, 1), cam)


def test_hsn_voc_background_and_mass_by_hand():
    Hbg = np.zeros((2, 2, 3))
    Hbg[1, :, 2] = [1.0, 2.0]  # X_bg = 3 at the last pixel of the LAST image
    got = ref.hsn_voc_background(Hbg)
    assert got.shape == (2, 3)
    assert np.allclose(got[1, 2], 0.075, atol=1e-15)  # expit(0) = 1/2
    assert np.allclose(np.delete(got.ravel(), 5), 0.15 / (1 + np.exp(-3.0)), atol=1e-15)  # image 0 sees image 1's maximum
    assert np.allclose(ref.hsn_voc_background(np.zeros((3, 4, 5))), 0.075, atol=1e-15)
    import scipy.special as scipy_special

    rng = np.random.default_rng(0)
    H = rng.random((3, 4, 50)) ** 2
    X = np.sum(H, axis=1)
    assert np.abs(ref.hsn_voc_background(H) - 0.15 * scipy_special.expit(np.max(X) - X)).max() <= 1e-15
    maps = np.zeros((3, 7))
    maps[0, 6] = 1e-30
    maps[2, 0] = 2.0
    assert ref.class_mass(maps).tolist() == [True, False, True]
