"""CPU: the float64 oracle of the classifier loss head and of the ROC thresholds (tests/cls_head_ref.py) against
sklearn.metrics.roc_curve, torch.autograd in double, hand-checkable facts and a direct evaluation of 01_train/utilities.py's
formulas; the .mat file cls_train.predict writes against the project's loader of optimalScoreThresh."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import cls_head_ref as ref
from wsscam import _lib, cls_train


def _sklearn_thresh(t, s):
    """get_optimal_thresholds' body for one class (utilities.py:100-110) -> (threshold, kept points)"""
    from sklearn.metrics import roc_curve

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # a class without positives or negatives: nan rates, argmin 0
        fprs, tprs, threshs = roc_curve(t, s)
        return threshs[np.argmin(abs(tprs - (1 - fprs)))], len(threshs)


@pytest.mark.parametrize("mode", ["continuous", "eighths", "mixed"])
def test_curve_restatement_equals_sklearn(mode):
    rng = np.random.default_rng({"continuous": 1, "eighths": 2, "mixed": 3}[mode])
    for _ in range(150):
        n = int(rng.integers(2, 300))
        t = (rng.random(n) < rng.uniform(0.05, 0.95)).astype(np.float32)
        if t.min() == t.max():
            t[0] = 1 - t[0]
        s = rng.random(n).astype(np.float32)
        if mode == "eighths":
            s = (np.round(s * 8) / 8).astype(np.float32)
        if mode == "mixed":
            s = (0.5 * s + 0.5 * t * rng.random(n)).astype(np.float32)
        thr, status, n_points, fps, tps = ref.roc_thresholds(s[:, None], t[:, None])
        want_thr, want_k = _sklearn_thresh(t, s)
        assert status[0] == 0 and n_points[0] == want_k
        assert thr[0] == np.float32(want_thr) and thr.dtype == np.float32
        assert fps[0, n_points[0] - 1] == n - t.sum() and tps[0, n_points[0] - 1] == t.sum()


def test_degenerate_classes_equal_sklearn():
    rng = np.random.default_rng(5)
    n = 40
    s = rng.random(n).astype(np.float32)
    for t, bit in ((np.zeros(n, np.float32), ref.NO_POSITIVE), (np.ones(n, np.float32), ref.NO_NEGATIVE)):
        thr, status, n_points, _, _ = ref.roc_thresholds(s[:, None], t[:, None])
        want_thr, want_k = _sklearn_thresh(t, s)
        assert np.isposinf(thr[0]) and np.isposinf(want_thr) and status[0] == bit and n_points[0] == want_k
    t = (rng.random(n) < 0.5).astype(np.float32)
    flat = np.full(n, 0.375, np.float32)  # all scores equal: both points at distance 1, the first one (+inf) wins
    thr, status, n_points, fps, tps = ref.roc_thresholds(flat[:, None], t[:, None])
    assert np.isposinf(thr[0]) and status[0] == 0 and n_points[0] == 2 == _sklearn_thresh(t, flat)[1]
    assert np.isposinf(_sklearn_thresh(t, flat)[0])
    # -0 and +0 are one score
    z = np.array([0.0, -0.0, 0.5, -0.0], np.float32)
    assert ref.roc_points(np.array([1, 0, 1, 0]), z)[2].tolist() == [np.inf, 0.5, 0.0]


def _torch_loss(feat, kind, w, bias, target, sample_w):
    f = torch.tensor(ref.f64(feat), requires_grad=True)
    wt = torch.tensor(ref.f64(w), requires_grad=True)
    C = w.shape[0]
    bt = torch.tensor(np.zeros(C) if bias is None else ref.f64(bias), requires_grad=True)
    z = torch.tensor(ref.f64(target))
    wts = torch.ones(f.shape[0], dtype=torch.float64) if sample_w is None else torch.tensor(ref.f64(sample_w))
    pooled = f.amax(dim=1) if kind == "max" else f.mean(dim=1)
    p = torch.sigmoid(pooled @ wt.T + bt)
    pc = torch.clamp(p, float(ref.EPS), float(ref.HI))
    ell = -(z * torch.log(pc) + (1 - z) * torch.log(1 - pc)).mean(dim=1)
    loss = (wts * ell).sum() / torch.count_nonzero(wts)
    return (loss,) + torch.autograd.grad(loss, [f, wt, bt])


@pytest.mark.parametrize("kind", ["mean", "max"])
@pytest.mark.parametrize("shape", [(3, 35, 64, 5), (1, 1, 4, 1), (4, 9, 256, 21)], ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradients_equal_autograd(kind, shape):
    """moderate logits: 1 - p in double costs 1e-16 / (1 - p) of relative error there, far inside 1e-9"""
    feat, w, bias, target, sample_w = ref.make_case(shape, kind)
    got = ref.cls_loss(feat, kind, w, bias, target, sample_w)
    assert np.abs(got["logit"]).max() < 25
    loss, g_f, g_w, g_b = _torch_loss(feat, kind, w, bias, target, sample_w)
    assert abs(got["values"]["loss"] - float(loss.detach())) <= 1e-9 * got["mag"]["loss"]
    for name, want in (("g_feat", g_f), ("g_w", g_w), ("g_bias", g_b)):
        want = want.numpy()
        assert np.abs(got[name] - want).max() <= 1e-9 * np.abs(want).max(), name


def test_tied_maxima_share_equally_as_amax_does():
    feat = np.zeros((2, 5, 4), np.float32)
    feat[0, :, 0] = 2.0           # all five positions
    feat[0, [1, 3], 1] = 1.0      # two of them
    feat[1, 2, :] = [3.0, -0.0, 1.0, 0.0]
    feat[1, 4, 1] = 0.0           # -0 and +0 tie with the other zeros of the column
    w = np.array([[1, -1, 2, 0], [0, 1, 1, -2]], np.float32)
    target = np.array([[1, 0], [0, 1]], np.float32)
    got = ref.cls_loss(feat, "max", w, None, target)
    assert got["ties"][0].tolist() == [5, 2, 5, 5] and got["ties"][1, 1] == 5
    _, g_f, g_w, _ = _torch_loss(feat, "max", w, None, target, None)
    assert np.abs(got["g_feat"] - g_f.numpy()).max() <= 1e-15
    assert np.abs(got["g_w"] - g_w.numpy()).max() <= 1e-15
    col = got["g_feat"][0, :, 1]
    assert col[1] == col[3] != 0 and col[0] == col[2] == col[4] == 0


def test_hand_checkable_facts():
    # p = 0.5 rounds to 0 (half to even): a zero logit predicts nothing and equals a zero target
    feat = np.zeros((2, 3, 4), np.float32)
    w = np.ones((2, 4), np.float32)
    target = np.array([[1, 0], [0, 0]], np.float32)
    v = ref.cls_loss(feat, "mean", w, None, target)
    assert (v["p"] == 0.5).all()
    assert v["values"]["predicted"] == 0 and v["values"]["tp"] == 0 and v["values"]["possible"] == 1 and v["values"]["n_equal"] == 3
    assert v["values"]["loss"] == pytest.approx(np.log(2.0), rel=1e-15)
    acc, f1 = ref.keras_ratios(v["values"], 4)
    assert acc == 0.75 and f1 == 0.0
    # saturated logits: p is clipped, the loss is -log(eps) or -log(1 - hi) where wrong, and the gradient is zero everywhere
    feat = np.full((2, 3, 4), 10.0, np.float32)
    w = np.array([[1, 1, 1, 1], [-1, -1, -1, -1]], np.float32)
    v = ref.cls_loss(feat, "mean", w, None, np.array([[1, 1], [0, 0]], np.float32))
    assert np.abs(v["logit"]).min() == 40.0
    assert not v["g_feat"].any() and not v["g_w"].any() and not v["g_bias"].any()
    right, wrong_hi, wrong_lo = -np.log(ref.HI), -np.log(1.0 - ref.HI), -np.log(ref.EPS)
    assert v["values"]["loss"] == pytest.approx(((right + wrong_lo) / 2 + (wrong_hi + (-np.log(1 - ref.EPS))) / 2) / 2, rel=1e-14)
    assert float(ref.HI) == 1.0 - 2.0 ** -23
    # a zero-weight sample drops out of both the sum and the divisor
    feat, w, bias, target, _ = ref.make_case((3, 35, 64, 5), "mean", with_weights=False)
    sw = np.array([2.0, 0.0, 0.5], np.float32)
    a = ref.cls_loss(feat, "mean", w, bias, target, sw)
    b = ref.cls_loss(feat[[0, 2]], "mean", w, bias, target[[0, 2]], sw[[0, 2]])
    assert a["values"]["loss"] == pytest.approx(b["values"]["loss"], rel=1e-14)
    assert not a["g_feat"][1].any()
    assert np.abs(a["g_w"] - b["g_w"]).max() <= 1e-15 * np.abs(b["g_w"]).max() + 1e-18


def test_every_gpu_case_has_its_margins():
    """tests/test_gpu_cls_head.py's random cases: make_case asserts that every p is 1e-6 away from 0.5 and from the clip bounds"""
    for shape in [(3, 35, 64, 5), (1, 1, 4, 1), (4, 9, 256, 21)]:
        for kind in ("mean", "max"):
            for with_bias in (True, False):
                ref.make_case(shape, kind, with_bias=with_bias)


def _utilities_metrics(target, predictions, thresholds):
    """get_thresholded_metrics_class and _overall, utilities.py:118-165, written out"""
    pt = predictions >= thresholds
    out = {}
    for name, ax in (("class", 0), ("overall", None)):
        cp, cn = np.sum(target == 1, ax), np.sum(target == 0, ax)
        tp, fp = np.sum((target == 1) & (pt == 1), ax), np.sum((target == 0) & (pt == 1), ax)
        tn, fn = np.sum((target == 0) & (pt == 0), ax), np.sum((target == 1) & (pt == 0), ax)
        total = pt.shape[0] if ax == 0 else np.prod(pt.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = {"tpr": tp / cp, "fpr": fp / cn, "tnr": tn / cn, "fnr": fn / cp, "acc": np.sum(target == pt, ax) / total,
                         "f1": (2 * tp) / (2 * tp + fp + fn)}
    return out


def test_metric_ratios_equal_utilities():
    scores, targets = ref.make_scores(400, 6, seed=3)
    thr = ref.roc_thresholds(scores, targets)[0]
    thr[4] = 0.5
    got = cls_train.threshold_ratios(ref.threshold_counts(scores, targets, thr), 400)
    want = _utilities_metrics(targets, scores, list(thr))
    for scope in ("class", "overall"):
        for k, v in want[scope].items():
            assert np.array_equal(np.asarray(got[scope][k]), np.asarray(v, np.float64), equal_nan=True), (scope, k)
    # the Keras metrics of the loss head
    vals = [0.7, 0.6, 13.0, 4.0, 6.0, 5.0]
    m = cls_train.keras_metrics(vals, 20)
    assert m["binary_accuracy"] == 13 / 20 and m["counts"] == {"n_equal": 13, "tp": 4, "possible": 6, "predicted": 5}
    assert m["f1"] == ref.keras_ratios(m["counts"], 20)[1]


def test_mat_round_trip_through_the_projects_loader(tmp_path, monkeypatch):
    """the file predict() writes (cls_train.write_thresholds, its one statement for it) read back by net.common.load_pretrained,
    which looks for <model_dir>/<tag>/<tag>.mat"""
    from wsscam.net import common

    thr = np.array([0.25, np.inf, 0.625, 0.5], np.float32)
    tag = "VOC2012_VGG16"
    path = cls_train.write_thresholds(str(tmp_path / tag), tag, thr)
    assert path == str(tmp_path / tag / (tag + ".mat")) and os.path.exists(path)
    seen = {}
    monkeypatch.setattr(common, "keras_h5_weight_list", lambda path: [])
    monkeypatch.setattr(common, "state_dict_from_keras_weights", lambda weights, t, root, bn, mat: seen.setdefault("mat", mat))
    common.load_pretrained(str(tmp_path), tag)
    assert np.array_equal(np.asarray(seen["mat"], np.float32), thr)


def test_bindings_and_slots():
    assert set(("wsc_cls_loss", "wsc_roc_thresholds", "wsc_cls_threshold_counts")) <= set(_lib.header_symbols())
    assert _lib.CLS_LOSS_SLOTS == ref.LOSS_KEYS and len(_lib.CLS_COUNT_SLOTS) == 5
    assert (_lib.ROC_NO_POSITIVE, _lib.ROC_NO_NEGATIVE) == (ref.NO_POSITIVE, ref.NO_NEGATIVE)
