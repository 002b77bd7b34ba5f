"""GPU: the classifier loss head and the ROC thresholds on the device (csrc/cls_head.hip: wsc_cls_loss, wsc_roc_thresholds,
wsc_cls_threshold_counts; wsscam.cls_train) against the float64 oracle tests/cls_head_ref.py.

Bounds (tests/test_gpu_seg_loss.py's, on the same argument: double on both sides, float32 outputs rounded once; DESIGN.md section 5
carries the measured errors next to them):
  loss values       |got - want| <= 1e-10 * sum|terms|
  gradients, scores |got - want| <= 2^-23 |want| + 1e-10 max|want|
  counts            exact
The random cases keep every p at least 1e-6 away from 0.5 and from both clip bounds (asserted by the oracle's make_case), so no
count and no clip mask can hide behind a double-level summation difference.  The tie case has exact logits (small integers), zero
logits (p = 0.5 rounds to 0) and maxima held by 2 and by n positions, whose shares are compared bit for bit among themselves.
Everything wsc_roc_thresholds and wsc_cls_threshold_counts return is an integer or a copy of a score: compared exactly."""
import numpy as np
import pytest
import scipy.io

from tests import cls_head_ref as ref
from wsscam import _lib, cls_train
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

SMALL = [(3, 35, 64, 5), (1, 1, 4, 1), (4, 9, 256, 21)]
VGG_HEAD = (2, 1681, 1024, 20)  # the real VGG16 head width on a 41 x 41 map
POOLS = {"mean": _lib.CLS_POOL_MEAN, "max": _lib.CLS_POOL_MAX}
LOSS_TOL = 1e-10
CANARY = np.float32(-777.25)
WANT_ALL = ("score", "feat", "w", "bias")


def _id(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def cases():
    """(shape, pool, with_bias, with_weights) -> (inputs, oracle result): computed on first use, shared, never modified"""
    store = {}

    def get(shape, kind, with_bias, with_weights):
        key = (shape, kind, with_bias, with_weights)
        if key not in store:
            inputs = ref.make_case(shape, kind, with_bias=with_bias, with_weights=with_weights)
            store[key] = (inputs, ref.cls_loss(inputs[0], kind, *inputs[1:]))
        return store[key]

    return get


def run(ctx, kind, feat, w, bias, target, sample_w, want=WANT_ALL):
    """one wsc_cls_loss on uploaded arrays -> {'loss' float64 [6], 'score', 'feat', 'w', 'bias'}; the four optional buffers start
    canary-filled and only a requested one is handed to the call"""
    B, n, F = feat.shape
    C = w.shape[0]
    blank = {"score": (B, C), "feat": (B, n, F), "w": (C, F), "bias": (C,)}
    with DeviceMaps.from_host(ctx, feat) as fd, DeviceMaps.from_host(ctx, w) as wd, DeviceMaps.from_host(ctx, target) as td, \
            DeviceMaps.from_host(ctx, np.zeros(C, np.float32) if bias is None else bias) as bd, \
            DeviceMaps(ctx, (len(_lib.CLS_LOSS_SLOTS),), np.float64) as loss:
        outs = {k: DeviceMaps.from_host(ctx, np.full(s, CANARY, np.float32)) for k, s in blank.items()}
        try:
            ptr = {k: (outs[k].ptr if k in want else None) for k in outs}
            _lib.cls_loss(ctx, fd.ptr, B, n, F, POOLS[kind], wd.ptr, None if bias is None else bd.ptr, C, td.ptr, sample_w, loss.ptr,
                          score_dev=ptr["score"], grad_feat_dev=ptr["feat"], grad_w_dev=ptr["w"], grad_bias_dev=ptr["bias"])
            res = {k: d.to_host() for k, d in outs.items()}
            res["loss"] = loss.to_host()
            return res
        finally:
            for d in outs.values():
                d.free()


def excess(got, want):
    """max of |got - want| - (2^-23 |want| + 1e-10 max|want|): <= 0 passes; and the largest error relative to max|want|"""
    err = np.abs(got.astype(np.float64) - want)
    top = np.abs(want).max()
    return float((err - (2.0 ** -23 * np.abs(want) + 1e-10 * top)).max()), float(err.max() / top) if top > 0 else 0.0


def check_against_oracle(tag, got, oracle, B, C):
    v, mag = oracle["values"], oracle["mag"]
    worst = 0.0
    for k, name in enumerate(("loss", "mean_loss")):
        err = abs(got["loss"][k] - v[name])
        worst = max(worst, err / mag[name])
        assert err <= LOSS_TOL * mag[name], (name, got["loss"][k], v[name], mag[name])
    assert [int(x) for x in got["loss"][2:]] == [v[k] for k in ("n_equal", "tp", "possible", "predicted")]
    assert all(float(x).is_integer() for x in got["loss"][2:])
    rel = {}
    for name, want in (("score", oracle["p"]), ("feat", oracle["g_feat"]), ("w", oracle["g_w"]), ("bias", oracle["g_bias"])):
        assert np.isfinite(got[name]).all()
        ex, rel[name] = excess(got[name], want)
        assert ex <= 0, (name, ex, rel[name])
    print("cls_loss %s: loss max |err| / sum|terms| %.3g (bound %.3g); max |err| / max|want|: score %.3g, g_feat %.3g, g_w %.3g, "
          "g_bias %.3g" % (tag, worst, LOSS_TOL, rel["score"], rel["feat"], rel["w"], rel["bias"]))


@pytest.mark.parametrize("with_weights", [True, False], ids=["weights", "ones"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("kind", list(POOLS))
@pytest.mark.parametrize("shape", SMALL, ids=_id)
def test_loss_and_gradients_vs_oracle(ctx, cases, shape, kind, with_bias, with_weights):
    inputs, oracle = cases(shape, kind, with_bias, with_weights)
    got = run(ctx, kind, *inputs)
    check_against_oracle("%s %s" % (kind, _id(shape)), got, oracle, shape[0], shape[3])
    if with_weights and shape[0] > 1:  # the sample of weight 0 receives +0.0, to the bit
        assert not got["feat"][shape[0] // 2].tobytes().strip(b"\0")
    # a second call on the same input: the same bytes
    again = run(ctx, kind, *inputs)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    with ctx.scratch_fill(0xFF):  # nor do they depend on what the call's scratch held before
        filled = run(ctx, kind, *inputs)
    assert all(got[k].tobytes() == filled[k].tobytes() for k in got)
    # each optional output alone has the bits it has beside the others, and a buffer that was not asked for keeps its canary
    for only in WANT_ALL:
        alone = run(ctx, kind, *inputs, want=(only,))
        assert alone["loss"].tobytes() == got["loss"].tobytes() and alone[only].tobytes() == got[only].tobytes()
        assert all((alone[k] == CANARY).all() for k in WANT_ALL if k != only)
    none = run(ctx, kind, *inputs, want=())
    assert none["loss"].tobytes() == got["loss"].tobytes() and all((none[k] == CANARY).all() for k in WANT_ALL)


def test_the_real_vgg16_head_width(ctx, cases):
    """41 x 41 x 1024 -> 20 classes, no bias (the VGG16 models' Dense layer has none): 27 position chunks, 4 channel tiles"""
    inputs, oracle = cases(VGG_HEAD, "mean", False, True)
    got = run(ctx, "mean", *inputs)
    check_against_oracle("mean %s" % _id(VGG_HEAD), got, oracle, VGG_HEAD[0], VGG_HEAD[3])
    assert run(ctx, "mean", *inputs)["feat"].tobytes() == got["feat"].tobytes()


def test_cls_loss_class_is_that_call(ctx, cases):
    shape = SMALL[0]
    inputs, oracle = cases(shape, "max", True, True)
    feat, w, bias, target, sw = inputs
    got = run(ctx, "max", *inputs)
    cl = cls_train.ClsLoss(ctx, "max", shape[3])
    res, grads = cl.grad_step(feat.reshape(3, 7, 5, 64), w, bias, target, sample_weight=sw)
    try:
        assert grads.feat.shape == (3, 7, 5, 64)
        assert np.array_equal(grads.feat.to_host().reshape(feat.shape), got["feat"])
        assert np.array_equal(grads.w.to_host(), got["w"]) and np.array_equal(grads.bias.to_host(), got["bias"])
    finally:
        for g in grads:
            g.free()
    assert [res["loss"], res["mean_loss"]] == got["loss"][:2].tolist()
    acc, f1 = ref.keras_ratios(oracle["values"], shape[0] * shape[3])
    assert res["binary_accuracy"] == acc and res["f1"] == f1 and res["counts"] == {k: oracle["values"][k] for k in res["counts"]}
    # device inputs are read in place and stay the caller's; loss_step is the same call without the gradients
    with DeviceMaps.from_host(ctx, feat) as fd, DeviceMaps.from_host(ctx, w) as wd, DeviceMaps.from_host(ctx, target) as td:
        assert cl.loss_step(fd, wd, bias, td, sample_weight=sw) == res
        assert fd.ptr is not None and wd.ptr is not None and td.ptr is not None
    for fn, word in ((lambda: cl.loss_step(feat, w[:, :32], bias, target), "w"), (lambda: cl.loss_step(feat, w, bias[:3], target), "bias"),
                     (lambda: cl.loss_step(feat, w, bias, target[:2]), "targets"), (lambda: cl.loss_step(feat[0, 0], w, bias, target), "feat")):
        with pytest.raises(ValueError) as ei:
            fn()
        assert word in str(ei.value)
    with pytest.raises(ValueError):
        cls_train.ClsLoss(ctx, "sum", 5)


@pytest.mark.parametrize("kind", list(POOLS))
def test_ties_round_to_even_and_split_the_maximum(ctx, kind):
    B, n, F, C = 3, 35, 8, 4
    feat = np.zeros((B, n, F), np.float32)
    if kind == "mean":
        feat[0] = [1, 2, 0, -1, 3, 0, 0, 1]     # constant over the positions: the mean is the integer itself
        feat[1] = [0, 0, 0, 0, 0, 0, 0, 0]
        feat[2] = [2, -2, 1, 1, 0, 0, -3, 0]
    else:
        feat[0, :, :] = -4.0
        feat[0, [3, 17], 0] = 1.0                # two positions hold the maximum
        feat[0, :, 1] = 2.0                      # all n of them
        feat[0, 9, 2:] = [0, -1, 3, 0, 0, 1]     # single maxima
        feat[1, :, :] = -0.0                     # every position holds the maximum 0 (-0 counts as +0) ...
        feat[1, ::2, :] = 0.0
        feat[2, :, :] = -5.0
        feat[2, [0, 34], :] = [2, -2, 1, 1, 0, 0, -3, 0]  # ... and the first and the last position share every maximum here
    w = np.array([[1, -1, 0, 0, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1, 1, -1], [0, 0, 0, 0, 0, 0, 0, 0], [2, 0, -1, 0, -1, 0, 0, 2]], np.float32)
    target = np.array([[1, 0, 1, 0], [0, 1, 0, 1], [1, 1, 0, 0]], np.float32)
    oracle = ref.cls_loss(feat, kind, w, None, target)
    assert np.array_equal(oracle["logit"], np.rint(oracle["logit"])) and (oracle["logit"] == 0).sum() >= 4  # exact, some p = 0.5
    got = run(ctx, kind, feat, w, None, target, None)
    check_against_oracle("%s ties" % kind, got, oracle, B, C)
    assert (got["score"][oracle["logit"] == 0] == 0.5).all()
    if kind == "max":
        assert sorted(set(oracle["ties"].reshape(-1).tolist())) == [1, 2, n]
        g = got["feat"]
        assert g[0, 3, 0] == g[0, 17, 0] != 0 and np.count_nonzero(g[0, :, 0]) == 2
        assert (g[0, :, 1] == g[0, 0, 1]).all() and g[0, 0, 1] != 0
        assert g[1].tobytes() == np.broadcast_to(g[1, 0], (n, F)).tobytes()  # -0 and +0 alike, to the bit
        assert np.array_equal(g[2, 0], g[2, 34]) and not g[2, 1:34].any()
        assert np.array_equal(got["feat"] != 0, oracle["g_feat"] != 0)
    else:
        assert got["feat"].tobytes() == np.broadcast_to(got["feat"][:, :1], feat.shape).tobytes()


@pytest.mark.parametrize("kind", list(POOLS))
def test_saturated_logits_are_clipped_and_send_no_gradient(ctx, kind):
    feat = np.full((2, 6, 4), 10.0, np.float32)
    w = np.array([[1, 1, 1, 1], [-1, -1, -1, -1], [1, 1, 1, 1]], np.float32)
    target = np.array([[1, 1, 0], [0, 0, 1]], np.float32)
    oracle = ref.cls_loss(feat, kind, w, None, target)
    assert (np.abs(oracle["logit"]) == 40).all()
    got = run(ctx, kind, feat, w, None, target, None)
    check_against_oracle("%s saturated" % kind, got, oracle, 2, 3)
    for k in ("feat", "w", "bias"):
        assert not got[k].tobytes().strip(b"\0"), k  # +0.0, to the bit


def test_limits_are_checked_before_any_launch(ctx):
    B, n, F, C = 2, 3, 8, 3
    sizes = [12, B * C, B * n * F, C * F, C, B * n * F, C * F, C, B * C]  # loss (six doubles as floats), score, g_feat, g_w, g_bias, inputs
    offs = np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])]) * 4 + 64  # 16-byte aligned sections
    with DeviceMaps.from_host(ctx, np.full((int(offs[-1]) // 4 + 16,), CANARY, np.float32)) as buf:
        base = (buf.ptr + 15) // 16 * 16
        loss, score, g_feat, g_w, g_bias, feat, w, bias, target = (base + int(o) for o in offs[:9])
        ones = np.ones(B, np.float32)

        def call(B=B, n=n, F=F, C=C, pool=0, feat=feat, w=w, target=target, loss=loss, sw=ones, g_feat=g_feat, g_w=g_w, score=score):
            _lib.check(ctx._lib.wsc_cls_loss(ctx.h, feat, B, n, F, pool, w, bias, C, target, None if sw is None else sw.ctypes.data, loss,
                                             score, g_feat, g_w, g_bias))

        bad = [
            (lambda: call(B=0), "B=0"), (lambda: call(B=1025), "B=1025"),
            (lambda: call(C=0), "C=0"), (lambda: call(C=65), "C=65"),
            (lambda: call(F=6), "F=6"), (lambda: call(F=4100), "F=4100"), (lambda: call(F=0), "F=0"),
            (lambda: call(n=0), "n=0"), (lambda: call(n=65537), "n=65537"),
            (lambda: call(pool=2), "pool=2"),
            (lambda: call(feat=None), "feat_dev"), (lambda: call(w=None), "w_dev"), (lambda: call(target=None), "target_dev"),
            (lambda: call(loss=None), "loss_dev"),
            (lambda: call(sw=np.array([1, -1], np.float32)), "sample_w_host[1]"),
            (lambda: call(sw=np.array([np.inf, 1], np.float32)), "sample_w_host[0]"),
            (lambda: call(sw=np.array([np.nan, 1], np.float32)), "sample_w_host[0]"),
            (lambda: call(sw=np.zeros(2, np.float32)), "non-zero"),
            (lambda: call(g_feat=feat), "grad_feat_dev overlaps feat_dev"),
            (lambda: call(g_w=w + 16), "grad_w_dev overlaps w_dev"),
            (lambda: call(score=target), "score_dev overlaps target_dev"),
            (lambda: call(g_w=g_feat), "grad_feat_dev overlaps grad_w_dev"),
            (lambda: call(g_feat=g_feat + 4), "aligned"),
        ]
        for fn, word in bad:
            with pytest.raises(_lib.WscError) as ei:
                fn()
            assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (word, str(ei.value))
        with pytest.raises(ValueError):
            _lib.cls_loss(ctx, feat, B, n, F, 0, w, bias, C, target, np.ones(3, np.float32), loss)
        for fn, word in ((lambda: _lib.roc_thresholds(ctx, feat, feat, 0, 1, loss, score), "N=0"),
                         (lambda: _lib.roc_thresholds(ctx, feat, feat, 16385, 1, loss, score), "N=16385"),
                         (lambda: _lib.roc_thresholds(ctx, feat, feat, 4, 65, loss, score), "C=65"),
                         (lambda: _lib.roc_thresholds(ctx, feat, feat, 4, 1, loss, score, fps_dev=g_feat), "together"),
                         (lambda: _lib.roc_thresholds(ctx, feat, None, 4, 1, loss, score), "target_dev"),
                         (lambda: _lib.cls_threshold_counts(ctx, feat, feat, 16385, 1, w, loss), "N=16385"),
                         (lambda: _lib.cls_threshold_counts(ctx, feat, feat, 4, 0, w, loss), "C=0"),
                         (lambda: _lib.cls_threshold_counts(ctx, feat, feat, 4, 1, None, loss), "thresh_dev")):
            with pytest.raises(_lib.WscError) as ei:
                fn()
            assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (word, str(ei.value))
        ctx.sync()
        assert (buf.to_host() == CANARY).all()  # nothing was launched


# ---- ROC -------------------------------------------------------------------------------------------------------------------------
# 5000 and 16384 samples are the two key-array sizes beyond the 64 KiB a launch gets by default (P = 8192 and P = 16384); the
# smaller one runs first, so a launch limit that was raised to the first call's size only would refuse the second
ROC_CASES = {"7x1": (7, 1, False), "400x20": (400, 20, False), "400x20-eighths": (400, 20, True), "1449x20": (1449, 20, False),
             "5000x2": (5000, 2, False), "16384x2": (16384, 2, False)}


@pytest.fixture(scope="module")
def roc_cases():
    """name -> (scores, targets, oracle tuple): classes 1 (no positives) and 2 (all scores equal) are degenerate where C >= 3"""
    out = {}
    for name, (N, C, grid) in ROC_CASES.items():
        scores, targets = ref.make_scores(N, C, seed=11, grid=grid)
        if N == 7:
            scores = np.array([[0.9], [0.4], [0.4], [0.7], [0.1], [0.4], [0.8]], np.float32)
            targets = np.array([[1], [0], [1], [1], [0], [0], [0]], np.float32)
        out[name] = (scores, targets, ref.roc_thresholds(scores, targets))
    return out


def run_roc(ctx, scores, targets, curves=True):
    N, C = scores.shape
    with DeviceMaps.from_host(ctx, scores) as sd, DeviceMaps.from_host(ctx, targets) as td, \
            DeviceMaps.from_host(ctx, np.full(C, CANARY, np.float32)) as thr, DeviceMaps.from_host(ctx, np.full(C, -7, np.int32)) as status, \
            DeviceMaps.from_host(ctx, np.full(C, -7, np.int32)) as n_points, \
            DeviceMaps.from_host(ctx, np.full((C, N + 1), -7, np.int32)) as fps, DeviceMaps.from_host(ctx, np.full((C, N + 1), -7, np.int32)) as tps, \
            DeviceMaps.from_host(ctx, np.full((C, 5), -7, np.int64)) as counts:
        _lib.roc_thresholds(ctx, sd.ptr, td.ptr, N, C, thr.ptr, status.ptr, n_points_dev=n_points.ptr if curves else None,
                            fps_dev=fps.ptr if curves else None, tps_dev=tps.ptr if curves else None)
        _lib.cls_threshold_counts(ctx, sd.ptr, td.ptr, N, C, thr.ptr, counts.ptr)
        return thr.to_host(), status.to_host(), n_points.to_host(), fps.to_host(), tps.to_host(), counts.to_host()


@pytest.mark.parametrize("name", list(ROC_CASES))
def test_roc_thresholds_and_counts_equal_the_oracle(ctx, roc_cases, name):
    scores, targets, want = roc_cases[name]
    N, C = scores.shape
    if C >= 3:
        assert want[1][1] == ref.NO_POSITIVE and np.isposinf(want[0][1]) and np.isposinf(want[0][2]) and want[2][2] == 2
        assert np.isfinite(np.delete(want[0], [1, 2])).all()
    if N == 7:  # by hand: groups 0.9 / 0.8 / 0.7 / 0.4 x 3 / 0.1; |tpr - (1 - fpr)| is smallest at 0.7 (tpr 2/3, fpr 1/4)
        assert want[0].tolist() == [np.float32(0.7)] and want[2].tolist() == [6]
    got = run_roc(ctx, scores, targets)
    for k, what in enumerate(("thresholds", "status", "n_points", "fps", "tps")):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), what
    assert np.array_equal(got[5], ref.threshold_counts(scores, targets, want[0]))
    print("roc %s: kept points per class %d .. %d of %d samples" % (name, want[2].min(), want[2].max(), N))
    # without the curve (and on scratch that held something else) the thresholds are the same and the three optional buffers
    # keep their fill
    with ctx.scratch_fill(0xFF):
        bare = run_roc(ctx, scores, targets, curves=False)
    assert np.array_equal(bare[0], want[0]) and np.array_equal(bare[1], want[1])
    assert all((bare[k] == -7).all() for k in (2, 3, 4))


def test_counts_at_given_thresholds(ctx, roc_cases):
    scores, targets, _ = roc_cases["400x20-eighths"]
    thr = np.linspace(-0.125, 1.125, 20).astype(np.float32)  # scores equal to a threshold count as predicted (>=)
    thr[3], thr[4] = np.inf, -np.inf
    with DeviceMaps.from_host(ctx, scores) as sd, DeviceMaps.from_host(ctx, targets) as td, DeviceMaps.from_host(ctx, thr) as th, \
            DeviceMaps(ctx, (20, 5), np.int64) as counts:
        _lib.cls_threshold_counts(ctx, sd.ptr, td.ptr, 400, 20, th.ptr, counts.ptr)
        got = counts.to_host()
    assert np.array_equal(got, ref.threshold_counts(scores, targets, thr))
    assert got[3, 0] == got[3, 1] == 0 and got[4, 2] == got[4, 3] == 0 and (got[:, :4].sum(axis=1) == 400).all()


def test_score_evaluator_in_three_uneven_batches_equals_one(ctx, roc_cases):
    scores, targets, want = roc_cases["1449x20"]
    N, C = scores.shape
    with cls_train.ScoreEvaluator(ctx, C) as one, cls_train.ScoreEvaluator(ctx, C) as three:
        one.update(scores, targets)
        for a, b in ((0, 1), (1, 700), (700, N)):
            if a == 1:  # one batch arrives on the device, as a forward pass leaves its scores
                with DeviceMaps.from_host(ctx, scores[a:b]) as sd:
                    three.update(sd, targets[a:b])
            else:
                three.update(scores[a:b], targets[a:b])
        assert one.N == three.N == N
        t1, t3 = one.thresholds(), three.thresholds()
        assert np.array_equal(t1, want[0]) and np.array_equal(t3, want[0]) and np.array_equal(three.status, want[1])
        p1, p3 = one.curve_points(), three.curve_points()
        assert all(np.array_equal(a, b) for a, b in zip(p1, p3)) and np.array_equal(p3[2], want[3]) and np.array_equal(p3[3], want[4])
        m1, m3 = one.metrics(t1), three.metrics(t3)
        counts = ref.threshold_counts(scores, targets, want[0])
        assert np.array_equal(m1["counts"], counts) and np.array_equal(m3["counts"], counts)
        want_m = cls_train.threshold_ratios(counts, N)
        for scope in ("class", "overall"):
            for k in want_m[scope]:
                assert np.array_equal(m3[scope][k], want_m[scope][k], equal_nan=True)
        fprs, tprs = three.curves()[0]
        k = int(want[2][0])
        assert len(fprs) == k and fprs[0] == tprs[0] == 0 and fprs[-1] == tprs[-1] == 1
        assert np.array_equal(tprs, want[4][0, :k] / np.float64(want[4][0, k - 1]))
        with pytest.raises(ValueError):
            three.update(scores[:, :3], targets[:, :3])
        with pytest.raises(ValueError):
            three.metrics(t3[:4])


def test_predict_writes_the_oracles_thresholds(ctx, roc_cases, tmp_path):
    val_s, val_t, val_want = roc_cases["400x20"]
    test_s, test_t, _ = roc_cases["400x20-eighths"]

    def batches(s, t, size):
        for a in range(0, len(s), size):
            yield s[a:a + size], t[a:a + size]

    sess = "VOC2012_VGG16"
    out = cls_train.predict(batches(val_s, val_t, 150), batches(test_s, test_t, 64), str(tmp_path / sess), sess, "test", ctx=ctx)
    mat = scipy.io.loadmat(out["mat_path"]).get("optimalScoreThresh")
    assert out["mat_path"] == str(tmp_path / sess / (sess + ".mat")) and mat.shape == (1, 20)
    assert np.array_equal(mat[0].astype(np.float32), val_want[0]) and np.array_equal(out["thresholds"], val_want[0])
    assert np.array_equal(out["status"], val_want[1])
    counts = ref.threshold_counts(test_s, test_t, val_want[0])
    assert np.array_equal(out["counts"], counts)
    want_m = cls_train.threshold_ratios(counts, 400)
    assert all(np.array_equal(out["overall"][k], want_m["overall"][k], equal_nan=True) for k in want_m["overall"])
    assert len(out["curves"]) == 20
    # eval_on = 'val' (VOC2012) evaluates the validation scores and never touches the test batches
    out_v = cls_train.predict(batches(val_s, val_t, 400), iter(()), str(tmp_path / sess), sess, "val", ctx=ctx)
    assert np.array_equal(out_v["counts"], ref.threshold_counts(val_s, val_t, val_want[0]))
    with pytest.raises(ValueError):
        cls_train.predict(batches(val_s, val_t, 400), iter(()), str(tmp_path / sess), sess, "train", ctx=ctx)
