"""CPU: the host arithmetic of wsscam.secdsrg.SegEvaluator -- ground-truth index preparation and the metrics of a (C+1) x (C+1)
confusion matrix -- against the literal restatement of 03a_sec-dsrg/model.py:698-719, :736-738 in tests/seg_eval_ref.py, and the
two entry points of csrc/seg_eval.hip in the export table.  No device: the matrix the device accumulates is formed with numpy."""
import numpy as np
import pytest

from tests import seg_eval_ref as ref
from wsscam import _lib, secdsrg


def _confusion(labels, gt_idx, C):
    """What wsc_label_confusion_nn accumulates with n_class = C + 1 and no ignored label: conf[gt][pred] += 1 per pixel."""
    conf = np.zeros((C + 1, C + 1), np.int64)
    for am, g in zip(labels, gt_idx):
        np.add.at(conf, (g.ravel().astype(np.int64), am.ravel()), 1)
    return conf


@pytest.mark.parametrize("C,use_colours", [(6, False), (6, True), (21, False), (21, True), (1, False)])
def test_metrics_equal_restated_loop(C, use_colours):
    rng = np.random.default_rng(100 + C + use_colours)
    colours = ref.colours_for(C) if use_colours else None
    absent = C - 2 if C > 2 else None  # in neither the ground truth nor the prediction
    labels, gts, idx = [], [], []
    for H, W in ((23, 31), (17, 17), (40, 12), (5, 4)):
        if absent is None:
            g = np.zeros((H, W), np.uint8)
            g[0, :] = 255
            am = np.zeros((H, W), np.int64)
        else:
            g = ref.make_gt_index(rng, H, W, C, absent)
            am = ref.make_labels(rng, H, W, C, absent)
        gt_img = ref.gt_as_image(g, colours)
        labels.append(am)
        gts.append(gt_img)
        idx.append(secdsrg.seg_gt_index(gt_img, C, colours))
        assert (g == 255).any() and (absent is None or not (g == absent).any() and not (am == absent).any())
        # both "no class" cases -- the 255 border, the unlisted colour -- are the extra index C
        assert idx[-1].dtype == np.uint8 and np.array_equal(idx[-1], np.where(g == 255, C, g))
    want = ref.finish(ref.count_loop(labels, gts, C, colours))
    got = secdsrg.seg_metrics_from_confusion(_confusion(labels, idx, C))
    ref.assert_metrics_equal(got, want)
    assert want["pred_count"].sum() == sum(a.size for a in labels)  # the no-class pixels are counted, not ignored
    assert want["gt_count"].sum() < want["pred_count"].sum()
    if absent is not None:
        assert got["IoU"][absent] == 0 and got["union"][absent] == 0
    assert isinstance(got["mIoU"], float) and got["mIoU"] == float(np.mean(want["intersect"] / (want["union"] + 1e-7)))


def test_gt_index_forms():
    C = 4
    plane = np.array([[0, 3, 255], [4, 1, 200]], np.uint8)
    want = np.array([[0, 3, C], [C, 1, C]], np.uint8)
    assert np.array_equal(secdsrg.seg_gt_index(plane, C), want)
    assert np.array_equal(secdsrg.seg_gt_index(np.repeat(plane[:, :, None], 3, 2), C), want)  # gt[:, :, 0]
    assert np.array_equal(secdsrg.seg_gt_index(plane.astype(np.int64) - (plane == 200) * 201, C), want)  # a negative index
    colours = ref.colours_for(C)
    rgb = ref.gt_as_image(want, colours)
    assert (rgb[0, 2] == np.asarray(ref.UNLISTED)).all()
    assert np.array_equal(secdsrg.seg_gt_index(rgb, C, colours), want)
    with pytest.raises(ValueError):
        secdsrg.seg_gt_index(rgb, C, colours[:-1])
    with pytest.raises(ValueError):
        secdsrg.seg_gt_index(np.zeros(5), C)


def test_names_of_precision_and_recall_are_the_references():
    """model.py:737-738: `precision` divides by gt_count, `recall` by pred_count."""
    conf = np.array([[5, 1, 0], [2, 7, 0], [3, 0, 0]], np.int64)
    m = secdsrg.seg_metrics_from_confusion(conf)
    assert np.array_equal(m["gt_count"], [6, 9]) and np.array_equal(m["pred_count"], [10, 8])
    assert np.array_equal(m["precision"], np.array([5.0, 7.0]) / (np.array([6.0, 9.0]) + 1e-5))
    assert np.array_equal(m["recall"], np.array([5.0, 7.0]) / (np.array([10.0, 8.0]) + 1e-5))
    assert np.array_equal(m["union"], [11, 10]) and np.array_equal(m["confusion_matrix"], conf[:2, :2])


def test_resize_f64_reference():
    rng = np.random.default_rng(5)
    m = rng.uniform(0.1, 1, (7, 9, 3))
    assert np.array_equal(ref.resize_f64(m, (7, 9)), m)  # identity
    up = ref.resize_f64(m, (14, 18))
    assert up.shape == (14, 18, 3)
    assert np.allclose(up[0, 0], m[0, 0]) and np.allclose(up[1, 1], 0.75 * 0.75 * m[0, 0] + 0.75 * 0.25 * (m[0, 1] + m[1, 0]) + 0.0625 * m[1, 1])
    assert np.allclose(ref.resize_f64(m[:1, :1], (5, 4)), m[0, 0])


def test_exports(built):
    declared = _lib.check_exports()
    assert "wsc_seg_unary_nhwc" in declared and "wsc_seg_resize_argmax" in declared
