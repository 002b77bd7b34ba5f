"""GPU: Model.predict kept on the device (csrc/seg_chain.hip, secdsrg.DeviceMaps / crf_layer_dev / SegNet.*_dev /
SegEvaluator on device maps and with crf=False / Predictor).

Every stage of the device chain that has a host twin is held to that twin's BITS (same kernels or the same arithmetic without FMA
contraction): preprocess, the zoomed CRF image, the forward pass, the resize of rescale_output, the evaluator.  Two stages are
held to bounds instead:
  the log-prob tail against the float64 restatement tests/seg_chain_ref.py: 4e-6 absolute.  The outputs lie in [ln(min_prob), 0] =
    [-9.21, 0] where the float32 spacing is 9.5e-7; clamp, sum and divide round at most (C + 2) 2^-24 relative on p, 1.4e-6 absolute
    on log p at C = 21; logf adds about 1 ulp and the final rounding: 4e-6 is about 1.5 times that total.
  output_dev against the host chain SegNet.output: the two differ in logf vs np.log inside the unaries and in the tail's sum
    order, so the difference is measured (exp(out), max|delta|) and asserted at 4 x the measured value, never above 1e-3, the
    project's dense-CRF tolerance (tests/test_gpu_crf.py test_crf_vs_oracle).  Measured values: next to the bound below and in
    DESIGN.md section 5."""
import numpy as np
import pytest

from tests import deeplab_ref, seg_chain_ref, seg_eval_ref
from wsscam import _lib, secdsrg
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}  # tests/test_gpu_deeplab.py's
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
THIN = ("DSRG", 5, (65, 65))
LOGPROB_TOL = 4e-6
# exp(output_dev) against exp(SegNet.output) on the thin DSRG case: measured max|delta| 5.27e-7 (MI355X; 1.77e-7 at seed
# size (7, 5)); the bound is 4 x that.  The log-prob tail measured 8.1e-7 / 1.19e-6 / 1.24e-6 on its three cases (bound 4e-6).
OUTPUT_MEASURED = 5.3e-7
OUTPUT_TOL = 4 * OUTPUT_MEASURED
CRF_TOL = 1e-3  # the project's dense-CRF tolerance: the ceiling of OUTPUT_TOL, and the bound where no measurement is pinned


def u8_rule(v):
    """image.astype(np.uint8) as include/wsscam.h defines it"""
    return np.asarray(v).astype(np.int32).astype(np.uint8)


@pytest.fixture(scope="module")
def thin():
    return deeplab_ref.thin_case(*THIN)


@pytest.fixture(scope="module")
def net(ctx, thin):
    n = secdsrg.SegNet("DSRG", thin[0], THIN[1], ctx=ctx)
    yield n
    n.close()


def _softmax_maps(rng, shape):
    e = np.exp(rng.normal(0, 2, shape))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


# ---- 1. preprocess ------------------------------------------------------------------------------------------------------------
def test_preprocess_dev_has_the_bits_of_preprocess(ctx, net):
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in ((37, 53), (64, 40), (48, 40))]
    want = net.preprocess(imgs, MEAN, size=(48, 40))
    with net.preprocess_dev(imgs, MEAN, size=(48, 40)) as x:
        assert x.shape == (3, 48, 40, 3) and x.dtype == np.float32
        got = x.to_host()
    assert np.array_equal(got, want)
    assert np.array_equal(got[2], imgs[2][:, :, ::-1].astype(np.float32) - MEAN)  # identity size: t == 0, exact
    # the float64 restatement: the resize rounds a few times at magnitude <= 255
    ref = np.stack([seg_chain_ref.preprocess(im, MEAN, (48, 40)) for im in imgs])
    assert np.abs(got - ref).max() <= 1e-6 * 255
    # keep_images: the packed batch comes back as it went up
    x, packed = net.preprocess_dev(imgs, MEAN, size=(48, 40), keep_images=True)
    try:
        assert packed.sizes == [(37, 53), (64, 40), (48, 40)] and packed.dtype == np.uint8
        assert np.array_equal(packed.to_host(), np.concatenate([im.reshape(-1) for im in imgs]))
        assert np.array_equal(x.to_host(), want)
    finally:
        x.free()
        packed.free()
    assert x.ptr is None
    with pytest.raises(ValueError):
        net.preprocess_dev([imgs[0].astype(np.float32)], MEAN)


# ---- 2. the zoomed CRF image ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [(48, 40), (7, 5)], ids=lambda s: "%dx%d" % s)
def test_crf_image_u8(ctx, net, seed):
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, (48, 40, 3), dtype=np.uint8), rng.integers(0, 256, (30, 61, 3), dtype=np.uint8)]
    x1 = net.preprocess(imgs, MEAN, size=(48, 40))
    x2 = x1.copy()
    planted = np.array([-1.5, 256.7, 1000.25], np.float32)
    for k in range(3):
        x2[0, 3 + k, 5, k] = planted[k] - MEAN[k]
    x2[1, 0, 0, :] = planted - MEAN  # (the corner: sampled at every seed size)
    for x in (x1, x2):
        want = u8_rule(net.resize(x + MEAN.reshape(1, 1, 1, 3), seed))
        with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps(ctx, (2,) + seed + (3,), np.uint8) as out:
            _lib.seg_crf_image_u8(ctx, xd.ptr, 2, 48, 40, MEAN, seed, out.ptr)
            got = out.to_host()
        assert np.array_equal(got, want)
        if seed == (48, 40):
            assert np.array_equal(got, seg_chain_ref.crf_image(x, MEAN, seed))  # identity size: no lerp rounds, the oracle exactly
    assert got[1, 0, 0].tolist() == [255, 0, 232]  # -1.5, 256.7, 1000.25 by the int32 rule
    if seed == (48, 40):
        assert [int(got[0, 3 + k, 5, k]) for k in range(3)] == [255, 0, 232]


# ---- 3. the log-prob tail ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7 * 9), (2, 21, 41 * 41), (1, 32, 300)], ids=lambda s: "%dx%dx%d" % s)
def test_crf_logprob_vs_oracle(ctx, shape):
    B, C, n = shape
    rng = np.random.default_rng(100 + C)
    q = np.ascontiguousarray(np.transpose(_softmax_maps(rng, (B, n, C)), (0, 2, 1)))
    q[0, 0, ::7] = 0.0
    q[0, C - 1, 1::5] = 5e-5
    q[B - 1, 1, 3] = 9.9e-5
    q[B - 1, :, 2] = 0.0       # a whole row below min_prob
    q[0, :, 4] = 1.0 / C       # a row of equal q
    with DeviceMaps.from_host(ctx, q) as qd, DeviceMaps(ctx, (B, n, C), np.float32) as out:
        _lib.seg_crf_logprob(ctx, qd.ptr, B, C, n, 1e-4, out.ptr)
        got = out.to_host()
    ref = seg_chain_ref.crf_logprob(q, 1e-4)
    err = np.abs(got.astype(np.float64) - ref).max()
    print("crf_logprob %s: max |err| vs float64 %.3g (bound %.3g)" % (shape, err, LOGPROB_TOL))
    assert np.isfinite(got).all() and err <= LOGPROB_TOL
    assert np.abs(np.exp(got.astype(np.float64)).sum(-1) - 1.0).max() <= 1e-5
    assert (got[0, 4] == got[0, 4, 0]).all() and (got[B - 1, 2] == got[B - 1, 2, 0]).all()  # equal q: equal outputs


def test_crf_logprob_unaligned_rows(ctx):
    """C % 4 == 0 but the output 4 bytes off a 16-byte boundary: the scalar stores, the same bits."""
    q = np.ascontiguousarray(np.transpose(_softmax_maps(np.random.default_rng(5), (1, 300, 8)), (0, 2, 1)))
    with DeviceMaps.from_host(ctx, q) as qd, DeviceMaps(ctx, (2400 + 4,), np.float32) as a, DeviceMaps(ctx, (2400 + 4,), np.float32) as b:
        _lib.seg_crf_logprob(ctx, qd.ptr, 1, 8, 300, 1e-4, a.ptr)
        _lib.seg_crf_logprob(ctx, qd.ptr, 1, 8, 300, 1e-4, b.ptr + 4)
        assert np.array_equal(a.to_host()[:2400], b.to_host()[1:2401])


# ---- 4. output_dev / rescale_output_dev against the host chain -----------------------------------------------------------------
def test_output_dev_vs_host_chain(ctx, net, thin):
    x = thin[1]
    host = net.output(x, MEAN, CRF_CFG)
    with net.output_dev(x, MEAN, CRF_CFG) as out:
        assert out.shape == host.shape == (2, 9, 9, 5)
        dev = out.to_host()
    delta = np.abs(np.exp(dev.astype(np.float64)) - np.exp(host.astype(np.float64))).max()
    print("output_dev vs SegNet.output: max |delta exp(out)| %.3g (bound %.3g = 4 x the measured %.3g)" % (delta, OUTPUT_TOL, OUTPUT_MEASURED))
    assert OUTPUT_TOL <= CRF_TOL
    assert delta <= OUTPUT_TOL
    assert np.abs(np.exp(dev.astype(np.float64)).sum(-1) - 1.0).max() <= 1e-5
    # a DeviceMaps input gives the bits of the host-array input (one upload either way)
    with DeviceMaps.from_host(ctx, x) as xd, net.output_dev(xd, MEAN, CRF_CFG) as out:
        assert np.array_equal(out.to_host(), dev)
        assert xd.ptr is not None  # the caller's buffer stays the caller's
    # pred()'s resize: the same kernel, the same bits
    with net.rescale_output_dev(x, MEAN, CRF_CFG) as resc:
        assert resc.shape == (2, 65, 65, 5)
        assert np.array_equal(resc.to_host(), net.resize(dev, (65, 65)))
    with net.rescale_output_dev(x, MEAN, CRF_CFG, size=(33, 70)) as resc:
        assert np.array_equal(resc.to_host(), net.resize(dev, (33, 70)))


def test_output_dev_at_another_seed_size(ctx, net, thin):
    """seed_size != the map's size: image and map go through the TF resize first.  Held to the dense-CRF tolerance (no measurement
    is pinned for this shape)."""
    x = thin[1]
    host = net.output(x, MEAN, CRF_CFG, seed_size=(7, 5))
    with net.output_dev(x, MEAN, CRF_CFG, seed_size=(7, 5)) as out:
        assert out.shape == (2, 7, 5, 5)
        dev = out.to_host()
    delta = np.abs(np.exp(dev.astype(np.float64)) - np.exp(host.astype(np.float64))).max()
    print("output_dev seed (7, 5) vs SegNet.output: max |delta exp(out)| %.3g" % delta)
    assert delta <= CRF_TOL
    with net.rescale_output_dev(x, MEAN, CRF_CFG, seed_size=(7, 5)) as resc:
        assert np.array_equal(resc.to_host(), net.resize(dev, (65, 65)))
    with net.output_dev(x, MEAN, CRF_CFG, seed_size=6) as out:
        assert out.shape == (2, 6, 6, 5)


def test_forward_dev_has_the_bits_of_forward(ctx, net, thin):
    x = thin[1]
    prob, fc8 = net.forward(x, want_fc8=True)
    p, f = net.forward_dev(x, want_fc8=True)
    with p, f:
        assert np.array_equal(p.to_host(), prob) and np.array_equal(f.to_host(), fc8)
    with DeviceMaps.from_host(ctx, x) as xd, net.softmax_dev(xd) as p:
        assert p.shape == (2, 9, 9, 5) and np.array_equal(p.to_host(), prob)


# ---- 5. the evaluator on device maps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resize_after_crf", [False, True])
def test_evaluator_on_device_maps(ctx, resize_after_crf):
    rng = np.random.default_rng(21)
    C, sizes = 5, ((20, 24), (33, 17))
    maps = _softmax_maps(rng, (2, 9, 11, C))
    imgs = [rng.integers(0, 256, ((9, 11) if resize_after_crf else hw) + (3,), dtype=np.uint8) for hw in sizes]
    gts = [seg_eval_ref.make_gt_index(rng, hw[0], hw[1], C, absent=3) for hw in sizes]
    a = secdsrg.SegEvaluator(C, CRF_CFG, resize_after_crf=resize_after_crf, ctx=ctx)
    b = secdsrg.SegEvaluator(C, CRF_CFG, resize_after_crf=resize_after_crf, ctx=ctx)
    c = secdsrg.SegEvaluator(C, CRF_CFG, resize_after_crf=resize_after_crf, ctx=ctx)
    try:
        want = a.update(list(maps), imgs, gts, want_pred=True)
        with DeviceMaps.from_host(ctx, maps) as md:
            got = b.update(md, imgs, gts, want_pred=True)
            assert md.ptr is not None
            # ... and with the images on the device too: a packed ragged batch
            packed = DeviceMaps.from_host(ctx, np.concatenate([im.reshape(-1) for im in imgs]))
            packed.sizes = [im.shape[:2] for im in imgs]
            packed.offsets = [0, imgs[0].size]
            with packed:
                got_c = c.update(md, packed, gts, want_pred=True)
        for w, g, g2 in zip(want, got, got_c):
            assert g.dtype == np.uint8 and np.array_equal(w, g) and np.array_equal(w, g2)
        ma, mb, mc = a.metrics(), b.metrics(), c.metrics()
        seg_eval_ref.assert_metrics_equal(mb, ma)
        seg_eval_ref.assert_metrics_equal(mc, ma)
        assert ma["pred_count"].sum() == sum(h * w for h, w in sizes)
        with pytest.raises(ValueError):
            with DeviceMaps.from_host(ctx, maps[:, :, :, :4]) as bad:
                b.update(bad, imgs, gts)
    finally:
        a.close()
        b.close()
        c.close()


# ---- 6. crf=False: the is_eval=False pass -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [False, True])
def test_evaluator_without_crf(ctx, colour):
    rng = np.random.default_rng(31)
    C = 5
    colours = seg_eval_ref.colours_for(C) if colour else None
    maps = _softmax_maps(rng, (2, 19, 23, C))  # 437 pixels: more than one block
    maps[0, 0, 0, :] = 0.2                    # every class ties: 0 wins
    maps[0, 1, 2, 1] = maps[0, 1, 2, 3] = 0.45  # two maxima: the first
    maps[0, 1, 2, [0, 2, 4]] = 0.1 / 3
    maps[1, 5, 5, 2] = maps[1, 5, 5, 4] = 0.5
    maps[1, 5, 5, [0, 1, 3]] = 0.0
    want = np.argmax(maps, -1)
    assert want[0, 0, 0] == 0 and want[0, 1, 2] == 1 and want[1, 5, 5] == 2
    gts = [seg_eval_ref.make_gt_index(rng, 19, 23, C, absent=1) for _ in range(2)]
    gt_imgs = [seg_eval_ref.gt_as_image(g, colours) for g in gts]
    ref = seg_eval_ref.finish(seg_eval_ref.count_loop(list(want), gt_imgs, C, colours))
    a = secdsrg.SegEvaluator(C, None, colours=colours, ctx=ctx, crf=False)
    b = secdsrg.SegEvaluator(C, CRF_CFG, colours=colours, ctx=ctx, crf=False)
    try:
        with DeviceMaps.from_host(ctx, maps) as md:
            got = a.update(md, None, gt_imgs if colour else gts, want_pred=True)
        for k in range(2):
            assert np.array_equal(got[k], want[k])
        seg_eval_ref.assert_metrics_equal(a.metrics(), ref)
        # the list form, ragged: the second image cropped to another size
        small = np.ascontiguousarray(maps[1, :7, :6])
        g_small = np.ascontiguousarray((gt_imgs if colour else gts)[1][:7, :6])
        got = b.update([maps[0], small], None, [(gt_imgs if colour else gts)[0], g_small], want_pred=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1, :7, :6])
        assert b.update([maps[0]], None, [gts[0] if not colour else gt_imgs[0]]) is None
        with pytest.raises(ValueError):  # map and ground truth share one size
            b.update([maps[0]], None, [(gt_imgs if colour else gts)[0][:10]])
    finally:
        a.close()
        b.close()


# ---- 7. Predictor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resize_after_crf", [False, True])
def test_predictor_is_the_manual_chain_and_moves_no_maps(ctx, net, thin, monkeypatch, resize_after_crf):
    rng = np.random.default_rng(41)
    C, size = THIN[1], THIN[2]
    batches = []
    for hws in (((70, 80), (65, 65)), ((50, 66), (90, 71), (65, 65))):
        imgs = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in hws]
        gts = [seg_eval_ref.make_gt_index(rng, hw[0], hw[1], C, absent=2) for hw in hws]
        batches.append((imgs, gts))
    # the manual chain on host arrays
    ev = secdsrg.SegEvaluator(C, CRF_CFG, resize_after_crf=resize_after_crf, ctx=ctx)
    want = []
    try:
        for imgs, gts in batches:
            x = net.preprocess(imgs, MEAN, size=size)
            prob = net.softmax(x)
            crf_imgs = list(u8_rule(net.resize(x, prob.shape[1:3]))) if resize_after_crf else imgs  # np.uint8(img[j]), :693
            want.append(ev.update(list(prob), crf_imgs, gts, want_pred=True))
        want_m = ev.metrics()
    finally:
        ev.close()
    pred = secdsrg.Predictor("DSRG", thin[0], C, CRF_CFG, MEAN, size=size, resize_after_crf=resize_after_crf, ctx=ctx)
    try:
        got = pred.update(batches[0][0], batches[0][1], want_pred=True)
        for w, g in zip(want[0], got):
            assert np.array_equal(w, g)
        # the second batch without want_pred, counting what crosses the bus
        ups, downs = [], []
        up0, down0 = ctx.to_device, ctx.to_host

        def to_device(arr, pooled=False):
            ups.append(np.asarray(arr).nbytes)
            return up0(arr, pooled=pooled)

        def to_host(buf, shape, dtype, offset_bytes=0):
            downs.append(int(np.prod(shape)) * np.dtype(dtype).itemsize)
            return down0(buf, shape, dtype, offset_bytes=offset_bytes)

        monkeypatch.setattr(ctx, "to_device", to_device)
        monkeypatch.setattr(ctx, "to_host", to_host)
        imgs, gts = batches[1]
        assert pred.update(imgs, gts) is None
        monkeypatch.undo()
        img_bytes, gt_bytes = sum(im.size for im in imgs), sum(g.size for g in gts)
        map_bytes = 3 * 9 * 9 * C * 4
        assert map_bytes > 4096  # (so the 4 KB allowance below cannot hide the maps)
        assert downs == []
        assert sorted(ups)[-2:] == sorted([img_bytes, gt_bytes]), ups  # the packed images and the ground truths, once each
        assert sum(ups) - img_bytes - gt_bytes <= 4096, ups
        seg_eval_ref.assert_metrics_equal(pred.metrics(), want_m)
    finally:
        pred.close()
    assert pred.net is None and pred.ev is None
    pred.close()  # idempotent


# ---- 8. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_are_checked_before_any_launch(ctx):
    buf = ctx.alloc(1 << 16, pooled=True)
    p = buf.ptr
    hw1, off1 = [(4, 4)], [0]
    bad = [
        # wsc_seg_preprocess_u8
        (lambda: _lib.seg_preprocess_u8(ctx, None, hw1, off1, MEAN, (4, 4), p), "img_dev"),
        (lambda: _lib.seg_preprocess_u8(ctx, p, hw1, off1, MEAN, (4, 4), None), "x_dev"),
        (lambda: _lib.seg_preprocess_u8(ctx, p, [], [], MEAN, (4, 4), p), "n="),
        (lambda: _lib.seg_preprocess_u8(ctx, p, [(0, 4)], off1, MEAN, (4, 4), p), "src_hw_host"),
        (lambda: _lib.seg_preprocess_u8(ctx, p, hw1, off1, MEAN, (4, 0), p), "W="),
        (lambda: _lib.seg_preprocess_u8(ctx, p, hw1, [-3], MEAN, (4, 4), p), "src_off_host"),
        # wsc_seg_crf_image_u8
        (lambda: _lib.seg_crf_image_u8(ctx, None, 1, 4, 4, MEAN, (4, 4), p), "x_dev"),
        (lambda: _lib.seg_crf_image_u8(ctx, p, 1, 4, 4, MEAN, (4, 4), None), "out_dev"),
        (lambda: _lib.seg_crf_image_u8(ctx, p, 0, 4, 4, MEAN, (4, 4), p), "B="),
        (lambda: _lib.seg_crf_image_u8(ctx, p, 65536, 4, 4, MEAN, (4, 4), p), "B="),
        (lambda: _lib.seg_crf_image_u8(ctx, p, 1, 0, 4, MEAN, (4, 4), p), "H="),
        (lambda: _lib.seg_crf_image_u8(ctx, p, 1, 4, 4, MEAN, (4, 0), p), "sw="),
        # wsc_seg_crf_logprob
        (lambda: _lib.seg_crf_logprob(ctx, None, 1, 4, 16, 1e-4, p), "q_dev"),
        (lambda: _lib.seg_crf_logprob(ctx, p, 1, 4, 16, 1e-4, None), "out_dev"),
        (lambda: _lib.seg_crf_logprob(ctx, p, 1, 33, 16, 1e-4, p), "C="),
        (lambda: _lib.seg_crf_logprob(ctx, p, 1, 0, 16, 1e-4, p), "C="),
        (lambda: _lib.seg_crf_logprob(ctx, p, 1, 4, 0, 1e-4, p), "n="),
        (lambda: _lib.seg_crf_logprob(ctx, p, 0, 4, 16, 1e-4, p), "B="),
        # wsc_seg_planes_from_nhwc
        (lambda: _lib.seg_planes_from_nhwc(ctx, None, 1, 4, 16, p), "src_dev"),
        (lambda: _lib.seg_planes_from_nhwc(ctx, p, 1, 33, 16, p), "C="),
        (lambda: _lib.seg_planes_from_nhwc(ctx, p, 1, 4, 0, p), "n="),
    ]
    try:
        for call, word in bad:
            with pytest.raises(_lib.WscError) as ei:
                call()
            assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (word, str(ei.value))
        ctx.sync()
    finally:
        buf.free()


def test_softmax_dev_reports_a_saturated_forward_once(ctx, net, thin):
    x = thin[1]
    with pytest.raises(_lib.WscError) as ei:
        net.softmax_dev(x * 1e4)
    assert ei.value.status == _lib.WSC_ERR_RANGE
    assert ctx.range_status() == 0  # reported once, scoped to the forward that raised it
    with net.softmax_dev(x) as p:
        assert np.array_equal(p.to_host(), net.softmax(x))
