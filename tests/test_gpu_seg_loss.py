"""GPU: the SEC / DSRG loss head on the device (csrc/seg_loss.hip, wsc_seg_loss; secdsrg.SegLoss, SegNet.loss_step_dev) against
the float64 oracle tests/seg_loss_ref.py.

Bounds (DESIGN.md section 5 carries the measured errors next to them):
  loss values  |got - want| <= 1e-10 * sum|terms|.  Both sides work in double on identical float32 inputs, so they differ by the
               summation order plus 1 ulp in log: about n C 2^-53 relative to the sum of magnitudes, 4e-12 at the largest case; the
               bound leaves a factor of 25 over that.
  gradients    |got - want| <= 2^-23 |want| + 1e-10 max|want|: one float32 rounding of a double value, plus the double-level
               cancellation in g_p - <g_p, s>.
The random cases carry no ties inside any (image, class) map (asserted), so the tie rule cannot hide behind a tolerance; the tie
cases are compared with the same bounds against the oracle's stable-argsort placement -- neighbouring rank weights differ by
0.4 %, far outside them -- and the maximum's share bit for bit."""
import numpy as np
import pytest

from tests import deeplab_ref
from tests import seg_loss_ref as ref
from wsscam import _lib, secdsrg
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

SHAPES = [(3, 7, 5, 5), (2, 41, 41, 21), (1, 1, 1, 2), (1, 128, 64, 2), (2, 9, 9, 32)]
METHODS = {"SEC": _lib.SEG_LOSS_SEC, "DSRG": _lib.SEG_LOSS_DSRG}
MIN_PROB = 1e-4
LOSS_TOL = 1e-10
CANARY = np.float32(-777.25)
CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}  # tests/test_gpu_seg_chain.py's
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)


def _id(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def cases():
    """shape -> (inputs, {method: oracle result}): computed once, shared, never modified"""
    out = {}
    for shape in SHAPES:
        inputs = ref.make_case(shape)
        out[shape] = (inputs, {m: ref.evaluate(m, *inputs, min_prob=MIN_PROB) for m in METHODS})
    return out


def run(ctx, method, prob, crf, cues, labels, want=("prob", "fc8"), min_prob=MIN_PROB):
    """one wsc_seg_loss on uploaded arrays -> (loss float64 [9], the g_p buffer, the g_z buffer); both buffers start canary-filled
    and only a requested one is handed to the call"""
    B, H, W, C = prob.shape
    w_fg, z_fg = secdsrg.rank_weights(H * W, secdsrg.SEC_Q_FG)
    w_bg, z_bg = secdsrg.rank_weights(H * W, secdsrg.SEC_Q_BG)
    sec = method == "SEC"
    blank = np.full(prob.shape, CANARY, np.float32)
    with DeviceMaps.from_host(ctx, prob) as p, DeviceMaps.from_host(ctx, crf) as q, DeviceMaps.from_host(ctx, cues) as cu, \
            DeviceMaps.from_host(ctx, labels) as lab, DeviceMaps(ctx, (len(ref.KEYS),), np.float64) as loss, \
            DeviceMaps.from_host(ctx, blank) as gp, DeviceMaps.from_host(ctx, blank) as gz:
        _lib.seg_loss(ctx, METHODS[method], p.ptr, q.ptr, cu.ptr, lab.ptr if sec else None, B, H, W, C, min_prob,
                      w_fg if sec else None, z_fg, w_bg if sec else None, z_bg, loss.ptr,
                      grad_prob_dev=gp.ptr if "prob" in want else None, grad_fc8_dev=gz.ptr if "fc8" in want else None)
        return loss.to_host(), gp.to_host(), gz.to_host()


def grad_excess(got, want):
    """max of |got - want| - (2^-23 |want| + 1e-10 max|want|): <= 0 passes; and the largest error relative to max|want|"""
    err = np.abs(got.astype(np.float64) - want)
    top = np.abs(want).max()
    return float((err - (2.0 ** -23 * np.abs(want) + 1e-10 * top)).max()), float(err.max() / top) if top > 0 else 0.0


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_losses_and_gradients_vs_oracle(ctx, cases, shape, method):
    inputs, oracle = cases[shape]
    want_loss, mag, want_gp, want_gz, _ = oracle[method]
    assert not ref.has_ties(inputs[0])
    loss, gp, gz = run(ctx, method, *inputs)  # both gradients in one call
    worst = 0.0
    for k, name in enumerate(ref.KEYS):
        err = abs(loss[k] - want_loss[name])
        if mag[name] > 0:
            worst = max(worst, err / mag[name])
        assert err <= LOSS_TOL * mag[name], (name, loss[k], want_loss[name], mag[name])
    ex_p, rel_p = grad_excess(gp, want_gp)
    ex_z, rel_z = grad_excess(gz, want_gz)
    print("seg_loss %s %s: loss max |err| / sum|terms| %.3g (bound %.3g); g_p max |err| / max|g_p| %.3g, g_z %.3g"
          % (method, _id(shape), worst, LOSS_TOL, rel_p, rel_z))
    assert np.isfinite(gp).all() and np.isfinite(gz).all()
    assert ex_p <= 0 and ex_z <= 0
    # a second call on the same input: the same bits
    loss2, gp2, gz2 = run(ctx, method, *inputs)
    assert loss.tobytes() == loss2.tobytes() and gp.tobytes() == gp2.tobytes() and gz.tobytes() == gz2.tobytes()
    # either gradient alone has the bits it has beside the other, and the buffer that was not asked for keeps its canary;
    # want_grad=None touches neither
    loss_p, gp_p, gz_p = run(ctx, method, *inputs, want=("prob",))
    loss_z, gp_z, gz_z = run(ctx, method, *inputs, want=("fc8",))
    loss_n, gp_n, gz_n = run(ctx, method, *inputs, want=())
    assert loss_p.tobytes() == loss_z.tobytes() == loss_n.tobytes() == loss.tobytes()
    assert np.array_equal(gp_p, gp) and (gz_p == CANARY).all()
    assert np.array_equal(gz_z, gz) and (gp_z == CANARY).all()
    assert (gp_n == CANARY).all() and (gz_n == CANARY).all()
    # SegLoss is that call
    sl = secdsrg.SegLoss(method, shape[3], min_prob=MIN_PROB, ctx=ctx)
    losses, g = sl(*inputs[:3], labels=inputs[3], want_grad="prob")
    with g:
        assert np.array_equal(g.to_host(), gp)
    losses_n, none = sl(*inputs[:3], labels=inputs[3], want_grad=None)
    assert none is None and losses_n == losses
    assert [losses[name] for name in ref.KEYS] == loss.tolist()


def test_ties_follow_the_stable_rank_and_split_the_maximum(ctx):
    shape = (3, 7, 5, 5)
    prob, crf, cues, labels = (a.copy() for a in ref.make_case(shape))
    n = 35
    maps, crf_m, cues_m = prob.reshape(3, n, 5), crf.reshape(3, n, 5), cues.reshape(3, n, 5)
    maps[0, :, 1] = 0.125                     # image 0 (all-positive): a constant foreground map
    labels[1, 2] = 1.0
    maps[1, 5:16, 2] = np.float32(0.3)       # a block of pixels at one value inside a ranked map ...
    maps[1, [2, 30, 31, 33], 0] = np.float32(1e-4)  # ... and a saturated floor in a background map (loss_3)
    assert not labels[2, 1:].any()             # image 2 is background only: every foreground class takes loss_2
    tied = [3, 9, 20]
    maps[2, :, 3] = np.minimum(maps[2, :, 3], np.float32(0.5))
    maps[2, tied, 3] = np.float32(0.9)        # three pixels share the maximum; no cue and one crf value there, so the rest of
    cues_m[2, tied, 3] = 0.0                  # their gradient is the same number too
    crf_m[2, tied, 3] = np.float32(-0.25)
    assert ref.has_ties(prob)
    want_loss, mag, want_gp, want_gz, parts = ref.evaluate("SEC", prob, crf, cues, labels, min_prob=MIN_PROB)
    loss, gp, gz = run(ctx, "SEC", prob, crf, cues, labels)
    for k, name in enumerate(ref.KEYS):
        assert abs(loss[k] - want_loss[name]) <= LOSS_TOL * mag[name], name
    assert grad_excess(gp, want_gp)[0] <= 0 and grad_excess(gz, want_gz)[0] <= 0
    # the constant map: rank = pixel index, so the weights grow with it, exactly as the oracle places them
    g = gp.reshape(3, n, 5)
    rest = want_gp - parts["loss_1"]
    l1 = g[0, :, 1].astype(np.float64) - rest.reshape(3, n, 5)[0, :, 1]
    assert (np.diff(l1) < 0).all()
    assert np.abs(l1 - parts["loss_1"].reshape(3, n, 5)[0, :, 1]).max() <= 2.0 ** -22 * np.abs(want_gp).max()
    # the block: its weights go out in pixel order
    block = g[1, 5:16, 2].astype(np.float64) - rest.reshape(3, n, 5)[1, 5:16, 2]
    assert (np.diff(block) < 0).all()
    # the maximum's share: equal to the bit across the tied pixels, and the oracle's third
    share = g[2, tied, 3]
    assert share[0] == share[1] == share[2]
    l2 = parts["loss_2"].reshape(3, n, 5)[2, :, 3]
    assert np.count_nonzero(l2) == 3 and l2[3] == l2[9] == l2[20] == pytest.approx((1 / 3) / 4 / (1 - np.float64(np.float32(0.9))) / 3, rel=1e-14)


def test_limits_are_checked_before_any_launch(ctx):
    n_el = 27  # (1, 3, 3, 3)
    with DeviceMaps.from_host(ctx, np.full((32 + 4 * n_el,), CANARY, np.float32)) as buf:
        loss, gp, gz = buf.ptr, buf.ptr + 128, buf.ptr + 128 + 4 * n_el  # [loss | g_p | g_z | inputs], all canary
        src = buf.ptr + 128 + 8 * n_el
        w = np.ones(9, np.float32)

        def call(method=_lib.SEG_LOSS_SEC, B=1, H=3, W=3, C=3, labels=src, prob=src, w_fg=w, n_w=None):
            tab = np.ones(H * W, np.float32) if n_w is None else n_w
            _lib.seg_loss(ctx, method, prob, src, src, labels, B, H, W, C, MIN_PROB, tab if w_fg is not None else None, 1.0, tab, 1.0,
                          loss, grad_prob_dev=gp, grad_fc8_dev=gz)

        bad = [
            (lambda: call(H=8193, W=1), "H=8193"),
            (lambda: call(H=128, W=65), "pixels"),
            (lambda: call(C=1), "C=1"),
            (lambda: call(C=33), "C=33"),
            (lambda: call(labels=None), "labels_dev"),
            (lambda: call(B=0), "B=0"),
            (lambda: call(method=2), "method=2"),
            (lambda: call(prob=None), "prob_dev"),
            (lambda: call(w_fg=None), "w_fg_host"),
            (lambda: call(method=_lib.SEG_LOSS_DSRG, C=33, labels=None), "C=33"),
        ]
        for fn, word in bad:
            with pytest.raises(_lib.WscError) as ei:
                fn()
            assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (word, str(ei.value))
        ctx.sync()
        assert (buf.to_host() == CANARY).all()  # nothing was launched


def test_segloss_names_the_argument_it_rejects(ctx):
    prob, crf, cues, labels = ref.make_case((3, 7, 5, 5))
    sl = secdsrg.SegLoss("SEC", 5, ctx=ctx)
    bad = [
        (lambda: sl(prob[..., :4], crf, cues, labels), "prob"),
        (lambda: sl(prob, crf[:, :6], cues, labels), "crf"),
        (lambda: sl(prob, crf, cues[:2], labels), "cues"),
        (lambda: sl(prob, crf, cues, labels[:, :4]), "labels"),
        (lambda: sl(prob, crf, cues), "labels"),
        (lambda: sl(prob, crf, cues, labels, want_grad="logits"), "want_grad"),
        (lambda: sl(prob, crf.astype(np.complex64), cues, labels), "crf"),
    ]
    for fn, word in bad:
        with pytest.raises(ValueError) as ei:
            fn()
        assert word in str(ei.value), (word, str(ei.value))
    with DeviceMaps.from_host(ctx, cues.astype(np.float64)) as c64:
        with pytest.raises(ValueError) as ei:
            sl(prob, crf, c64, labels)
        assert "cues" in str(ei.value)
    with pytest.raises(ValueError):
        secdsrg.SegLoss("MCG", 5, ctx=ctx)
    with pytest.raises(ValueError):
        secdsrg.SegLoss("SEC", 1, ctx=ctx)
    # device maps are read in place and stay the caller's; (B, 1, 1, C) labels are the reference's shape; DSRG needs no labels
    with DeviceMaps.from_host(ctx, prob) as p, DeviceMaps.from_host(ctx, crf) as q, DeviceMaps.from_host(ctx, cues) as cu:
        a, ga = sl(p, q, cu, labels.reshape(3, 1, 1, 5))
        b, gb = sl(prob, crf, cues, labels)
        with ga, gb:
            assert a == b and set(a) == set(ref.KEYS) and all(isinstance(v, float) for v in a.values())
            assert ga.shape == prob.shape and np.array_equal(ga.to_host(), gb.to_host())
        assert p.ptr is not None and q.ptr is not None and cu.ptr is not None
        d, gd = secdsrg.SegLoss("DSRG", 5, ctx=ctx)(p, q, cu)
        gd.free()
        assert d["expand"] == 0.0 and d["seed"] == d["seed_bg"] + d["seed_fg"]
    assert list(sl._weights) == [35]  # the tables are cached per n


@pytest.mark.parametrize("method", ["DSRG", "SEC"])
def test_loss_step_dev_is_the_manual_chain(ctx, method, monkeypatch):
    C = 5
    weights, x = deeplab_ref.thin_case(method, C, (65, 65))
    rng = np.random.default_rng(77)
    cues = (rng.random((2, 9, 9, C)) < 0.2).astype(np.float32)
    tags = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 1]], np.float32)
    net = secdsrg.SegNet(method, weights, C, ctx=ctx)
    try:
        # the manual chain, stage by stage
        with net.forward_dev(x) as prob, DeviceMaps.from_host(ctx, x) as xd:
            with secdsrg.crf_layer_dev(prob, xd, MEAN, CRF_CFG, C, min_prob=net.min_prob, ctx=ctx) as crf:
                grown = secdsrg.generate_seed_step(tags, cues, prob.to_host(), ctx=ctx) if method == "DSRG" else cues
                want, want_g = secdsrg.SegLoss(method, C, min_prob=net.min_prob, ctx=ctx)(prob, crf, grown, labels=tags)
                want_g_host = want_g.to_host()
                want_g.free()
        handed = []
        alloc0 = ctx.alloc

        def alloc(nbytes, pooled=False):
            handed.append(alloc0(nbytes, pooled=pooled))
            return handed[-1]

        monkeypatch.setattr(ctx, "alloc", alloc)
        losses, grad, new_cues = net.loss_step_dev(x, cues, tags, MEAN, CRF_CFG)
        assert losses == want  # to the bits
        assert np.array_equal(grad.to_host(), want_g_host)
        assert new_cues.shape == (2, 9, 9, C) and np.array_equal(new_cues.to_host(), grown)
        if method == "DSRG":
            assert grown.sum() >= cues.sum() and np.array_equal(np.maximum(grown, cues), grown)
        grad.free()
        new_cues.free()
        assert handed and all(b.ptr is None for b in handed)  # every buffer of the step went back
        # device inputs stay the caller's; want_grad reaches SegLoss
        del handed[:]
        with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, cues) as cd:
            mine = list(handed)
            del handed[:]
            l2, g2, nc2 = net.loss_step_dev(xd, cd, tags, MEAN, CRF_CFG, want_grad=None)
            assert l2 == want and g2 is None and xd.ptr is not None and cd.ptr is not None
            assert (nc2 is cd) == (method == "SEC")
            if nc2 is not cd:
                nc2.free()
            assert all(b.ptr is None for b in handed)
            # a failure inside the step frees what it had taken
            del handed[:]
            with pytest.raises(ValueError):
                net.loss_step_dev(xd, cd, tags, MEAN, CRF_CFG, seed_size=(7, 5))
            assert handed and all(b.ptr is None for b in handed)
            assert all(b.ptr is not None for b in mine)
        monkeypatch.undo()
    finally:
        net.close()
