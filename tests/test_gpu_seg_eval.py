"""GPU: the SEC / DSRG prediction tail on the device -- wsc_seg_unary_nhwc, wsc_seg_resize_argmax (csrc/seg_eval.hip) and the
driver wsscam.secdsrg.SegEvaluator -- against the library's own pieces taken one image at a time (wsc_bilinear_resize,
misc.imutils.crf_inference) and the numpy restatement of 03a_sec-dsrg/model.py:698-719 in tests/seg_eval_ref.py.

Tolerances (none is derived from the code under test):
  unaries  |U - (-log(float64(R)))| <= 2e-6 with R the wsc_bilinear_resize plane: the bound the project holds its -log unaries to
           (tests/test_gpu_hsn.py); here U < 8, one binade whose ulp is 4.8e-7, and the only freedom is the device logf.  Against the float64 resize:
           |exp(-U) - R64| <= 1.2e-5 = the project's 1e-5 for fp32 source coordinates on O(1) maps + the 2e-6 above.
  labels   equal on every pixel whose top-2 margin in the reference marginals exceeds 2e-3 = twice the project's max|dQ| <= 1e-3
           CRF bound; such low-margin pixels may be at most 0.5 % of all (the project's 99.5 % label figure).
  metrics  exact, on the evaluator's own labels."""
import numpy as np
import pytest

from tests import helpers
from tests import seg_eval_ref as ref
from wsscam import _lib, secdsrg
from wsscam.misc import imutils
from wsscam.voc12.dataloader import resize_bilinear_u8

pytestmark = pytest.mark.gpu

VOC_TEST = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 10}  # SEC.py:20
ADP_MORPH_TEST = {"g_sxy": 1, "g_compat": 20, "bi_sxy": 10, "bi_srgb": 40, "bi_compat": 50, "iterations": 5}  # SEC.py:24-25
MARGIN, LOW_MARGIN_SHARE = 2e-3, 0.005


def _softmax_hwc(rng, h, w, C):
    return np.ascontiguousarray(np.transpose(helpers.synth_crf_case(rng, h, w, C)[2], (1, 2, 0)), dtype=np.float32)


def _resize_planes(ctx, planes, out_hw):
    """wsc_bilinear_resize of (C, h, w) -> (C, H, W), fetched."""
    C, h, w = planes.shape
    dst = ctx.alloc(C * out_hw[0] * out_hw[1] * 4)
    _lib.bilinear_resize(ctx, ctx.to_device(np.ascontiguousarray(planes, dtype=np.float32)), C, h, w, dst, out_hw[0], out_hw[1])
    return ctx.to_host(dst, (C,) + tuple(out_hw), np.float32)


def _offsets(counts):
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


@pytest.mark.parametrize("C", [3, 5, 21, 32])
def test_unary_bits(ctx, C):
    """One call over the ragged batch.  C = 5 breaks the 16-byte alignment of a pixel's row, C = 32 is the limit."""
    rng = np.random.default_rng(700 + C)
    maps = [_softmax_hwc(rng, h, w, C) for (h, w), _ in ref.SIZES]
    src_hw = [s for s, _ in ref.SIZES]
    out_hw = [o for _, o in ref.SIZES]
    p_off = _offsets([m.size for m in maps])
    u_off = _offsets([C * H * W for H, W in out_hw])
    guard = 64
    u_dev = ctx.alloc((int(u_off[-1]) + guard) * 4)
    _lib.check(ctx._lib.wsc_memset(ctx.h, u_dev.ptr, 0xff, (int(u_off[-1]) + guard) * 4))  # every cell must be written
    _lib.seg_unary_nhwc(ctx, ctx.to_device(np.concatenate([m.reshape(-1) for m in maps])), C, src_hw, out_hw, p_off[:-1], u_off[:-1],
                        u_dev)
    flat = ctx.to_host(u_dev, (int(u_off[-1]) + guard,), np.float32)
    assert np.isnan(flat[int(u_off[-1]):]).all()  # nothing past the last block
    for b, m in enumerate(maps):
        H, W = out_hw[b]
        U = flat[u_off[b]:u_off[b + 1]].reshape(C, H, W)
        R = _resize_planes(ctx, np.transpose(m, (2, 0, 1)), (H, W))
        if src_hw[b] == out_hw[b]:
            assert np.array_equal(R, np.transpose(m, (2, 0, 1)))  # equal sizes: the map passes through
        assert R.min() > np.exp(-8.0) and np.isfinite(U).all()  # a condition on the inputs: U < 8
        d_log = np.abs(U.astype(np.float64) + np.log(R.astype(np.float64))).max()
        d_f64 = np.abs(np.exp(-U.astype(np.float64)) - np.transpose(ref.resize_f64(m, (H, W)), (2, 0, 1))).max()
        print("C=%d %r -> %r: |U + log R| %.3g, |exp(-U) - R64| %.3g, U max %.3f" % (C, src_hw[b], out_hw[b], d_log, d_f64, U.max()))
        assert d_log <= 2e-6, (b, d_log)
        assert d_f64 <= 1.2e-5, (b, d_f64)


@pytest.mark.parametrize("C,tie", [(3, False), (7, True), (32, False)])
def test_resize_argmax(ctx, C, tie):
    """Labels = np.argmax over the wsc_bilinear_resize planes (one sampler: same bits, same labels); with `tie` classes 2 and 4
    share one plane that holds the maximum everywhere, and the lower index wins."""
    rng = np.random.default_rng(800 + C)
    qs = []
    for (h, w), _ in ref.SIZES:
        q = np.ascontiguousarray(helpers.synth_crf_case(rng, h, w, C)[2], dtype=np.float32)  # (C, h, w)
        if tie:
            q[2] = q[4] = q.max(0) + np.float32(0.125)
        qs.append(q)
    src_hw = [s for s, _ in ref.SIZES]
    out_hw = [o for _, o in ref.SIZES]
    q_off = _offsets([q.size for q in qs])
    l_off = _offsets([H * W for H, W in out_hw])
    guard = 64
    l_dev = ctx.alloc((int(l_off[-1]) + guard) * 4)
    _lib.check(ctx._lib.wsc_memset(ctx.h, l_dev.ptr, 0xff, (int(l_off[-1]) + guard) * 4))
    _lib.seg_resize_argmax(ctx, ctx.to_device(np.concatenate([q.reshape(-1) for q in qs])), C, src_hw, out_hw, q_off[:-1], l_off[:-1],
                           l_dev)
    flat = ctx.to_host(l_dev, (int(l_off[-1]) + guard,), np.int32)
    assert (flat[int(l_off[-1]):] == -1).all()
    for b, q in enumerate(qs):
        lab = flat[l_off[b]:l_off[b + 1]].reshape(out_hw[b])
        want = np.argmax(_resize_planes(ctx, q, out_hw[b]), axis=0)
        assert np.array_equal(lab, want), (b, int((lab != want).sum()))
        if tie:
            assert (lab == 2).all()


def _eval_case(rng, C, colours, sizes, big_image=None):
    """sizes: [((h, w), (H, W))] map -> ground truth.  Image b has its ground truth's size, except `big_image`, which is larger
    (cv2.resize of the image is then on the path).  The ground truth is an unrelated draw with one class absent and a 255 border."""
    probs, images, gts = [], [], []
    for b, ((h, w), (H, W)) in enumerate(sizes):
        probs.append(_softmax_hwc(rng, h, w, C))
        ih, iw = (H + H // 2, W + W // 2 + 1) if b == big_image else (H, W)
        images.append(helpers.synth_crf_case(rng, ih, iw, 2)[0])
        gts.append(ref.gt_as_image(ref.make_gt_index(rng, H, W, C, absent=C - 2), colours))
    return probs, images, gts


def _check_labels(labels, q_refs, what):
    """q_refs[b]: (H, W, C) reference marginals.  Equal labels wherever the reference's top-2 margin exceeds MARGIN, and few
    pixels below it."""
    low = total = 0
    for b, (lab, q) in enumerate(zip(labels, q_refs)):
        H, W, C = q.shape
        qc = np.transpose(q, (2, 0, 1)).reshape(C, -1)
        sure = helpers.top2_margin(qc) > MARGIN
        want = np.argmax(qc, axis=0)
        assert lab.shape == (H, W) and lab.dtype == np.uint8
        bad = (lab.reshape(-1) != want) & sure
        assert not bad.any(), (what, b, int(bad.sum()))
        low += int((~sure).sum())
        total += sure.size
    print("%s: %d of %d pixels below the %.0e margin (%.4f %%)" % (what, low, total, MARGIN, 100.0 * low / total))
    assert low <= LOW_MARGIN_SHARE * total, (what, low, total)


EVAL_SIZES = (((21, 27), (47, 61)), ((33, 33), (50, 37)), ((21, 27), (47, 61)), ((40, 40), (25, 31)), ((17, 19), (17, 19)))


@pytest.mark.parametrize("C,cfg,use_colours", [(6, VOC_TEST, False), (21, ADP_MORPH_TEST, True)], ids=["voc6", "adp21"])
def test_evaluator(ctx, C, cfg, use_colours):
    """Five images, two of one size (four CRF groups), image 1 larger than its ground truth."""
    rng = np.random.default_rng(900 + C)
    colours = ref.colours_for(C) if use_colours else None
    probs, images, gts = _eval_case(rng, C, colours, EVAL_SIZES, big_image=1)
    keep = [p.copy() for p in probs], [im.copy() for im in images], [g.copy() for g in gts]
    ev = secdsrg.SegEvaluator(C, cfg, colours=colours, ctx=ctx)
    try:
        first = ev.update(probs[:2], images[:2], gts[:2], want_pred=True)
        labels = ev.update(probs, images, gts, want_pred=True)
        for got, orig in zip((probs, images, gts), keep):
            assert all(np.array_equal(a, b) for a, b in zip(got, orig))  # the inputs are not modified
        # the reference path, one image at a time: the device-resized map, the resized image, the per-image CRF mirror
        q_refs = []
        for b, (_, (H, W)) in enumerate(EVAL_SIZES):
            R = np.transpose(_resize_planes(ctx, np.transpose(probs[b], (2, 0, 1)), (H, W)), (1, 2, 0))
            img = images[b] if images[b].shape[:2] == (H, W) else resize_bilinear_u8(images[b], (H, W))
            q_refs.append(imutils.crf_inference(img, cfg, C, R, use_log=True, ctx=ctx))
        _check_labels(labels, q_refs, "C=%d" % C)
        # independent of ties: the counts of the evaluator's own labels, the second update on top of the first
        want = ref.finish(ref.count_loop(first + labels, gts[:2] + gts, C, colours))
        ref.assert_metrics_equal(ev.metrics(), want)
        assert want["gt_count"][C - 2] == 0 and want["pred_count"].sum() > want["gt_count"].sum()
    finally:
        ev.close()


def test_evaluator_resize_after_crf(ctx):
    """The DeepGlobe branch: CRF at the network size, the marginals resized, arg-max."""
    C, cfg = 7, VOC_TEST
    sizes = (((21, 27), (47, 61)), ((16, 16), (40, 40)))
    rng = np.random.default_rng(977)
    colours = ref.colours_for(C)
    probs, _, gts = _eval_case(rng, C, colours, sizes)
    images = [helpers.synth_crf_case(rng, h, w, 2)[0] for (h, w), _ in sizes]  # np.uint8(img[j]) at the network size
    ev = secdsrg.SegEvaluator(C, cfg, colours=colours, resize_after_crf=True, ctx=ctx)
    try:
        labels = ev.update(probs, images, gts, want_pred=True)
        q_refs = [ref.resize_f64(imutils.crf_inference(images[b], cfg, C, probs[b], use_log=True, ctx=ctx), sizes[b][1])
                  for b in range(len(sizes))]
        _check_labels(labels, q_refs, "resize_after_crf")
        ref.assert_metrics_equal(ev.metrics(), ref.finish(ref.count_loop(labels, gts, C, colours)))
        with pytest.raises(ValueError):  # the image has the map's size in this branch
            ev.update(probs, [np.zeros((47, 61, 3), np.uint8), images[1]], gts)
    finally:
        ev.close()


def test_argument_errors(ctx):
    """C = 33, a zero size and a NULL buffer: WSC_ERR_INVALID before any launch, outputs untouched, the stream clean."""
    n = 4096
    src = ctx.to_device(np.full(n, 0.5, np.float32))
    out = ctx.alloc(n * 4)
    _lib.check(ctx._lib.wsc_memset(ctx.h, out.ptr, 0x5a, n * 4))
    for fn in (_lib.seg_unary_nhwc, _lib.seg_resize_argmax):
        for kw, word in ((dict(C=33), "C=33"), (dict(C=0), "C=0"), (dict(src_hw=[(0, 4)]), "0x4"), (dict(out_hw=[(4, 0)]), "4x0"),
                         (dict(src=None), "null"), (dict(out=None), "null"), (dict(src_off=[-4]), "negative")):
            a = dict(src=src, C=3, src_hw=[(4, 4)], out_hw=[(8, 8)], src_off=[0], dst_off=[0], out=out)
            a.update(kw)
            with pytest.raises(_lib.WscError) as ei:
                fn(ctx, a["src"], a["C"], a["src_hw"], a["out_hw"], a["src_off"], a["dst_off"], a["out"])
            assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (fn.__name__, kw, str(ei.value))
    ctx.sync()
    assert (ctx.to_host(out, (n * 4,), np.uint8) == 0x5a).all()
    with pytest.raises(ValueError):
        secdsrg.SegEvaluator(33, VOC_TEST, ctx=ctx)


def _idle_pooled(ctx):
    return sum(len(v) for v in getattr(ctx, "_pool", {}).values())


def test_no_leaks(ctx):
    """Every pooled block an update takes is back in the context's pool when it returns, the matrix after close()."""
    rng = np.random.default_rng(31)
    C = 4
    sizes = EVAL_SIZES[:2]
    probs, images, gts = _eval_case(rng, C, None, sizes, big_image=0)
    small = [helpers.synth_crf_case(rng, h, w, 2)[0] for (h, w), _ in sizes]

    def run(want_pred, resize_after_crf):
        ev = secdsrg.SegEvaluator(C, VOC_TEST, resize_after_crf=resize_after_crf, ctx=ctx)
        try:
            before = _idle_pooled(ctx)
            out = ev.update(probs, small if resize_after_crf else images, gts, want_pred=want_pred)
            assert (out is not None) == want_pred  # nothing comes back per batch without want_pred
            during = _idle_pooled(ctx)
        finally:
            ev.close()
        return before, during, _idle_pooled(ctx)

    for mode in ((True, False), (False, True)):
        run(*mode)  # warm: the pool now holds a block of every size this shape asks for
        start = _idle_pooled(ctx)
        before, during, after = run(*mode)
        assert before == start - 1 and during == before and after == start, (mode, start, before, during, after)
