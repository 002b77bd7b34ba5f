"""GPU: the SEC / DSRG DeepLab-VGG16 forward pass (03a_sec-dsrg) against the float64 oracle tests/deeplab_ref.py: dilated
single layers, the TF-SAME pools, fc8-softmax, the TF bilinear resize, thin and full-width nets end to end, secdsrg.SegNet.

Bounds.  Dilation changes addresses, not arithmetic: the dilated layers are held to the bounds the undilated layers of each
precision already have (tests/test_gpu_conv.py: f16x3 4e-6 max|ref|, bf16x3 1e-4 max|ref|, f16 2^-11 |ref| + 3e-4 max|ref| on
half-rounded operands; tests/test_gpu_f32.py: the derived fma-chain bound (K + 8) 2^-24 A).  Nets: fc8 logits within 1e-4 of the
map's max in f16x3 (the bound of the f16x3 nets in tests/test_gpu_net.py) and 2e-5 in f32 (tests/test_gpu_f32.py's VGG16 bound);
softmax 1e-4 absolute; arg-max agreement 99.5 % (tests/test_deeplab_oracle.py checks on the CPU that the oracle's own float32
stays far inside all three for these seeds: <= 1.4e-6, <= 2.1e-6, 100 %).  Measured maxima: DESIGN.md section 5."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import deeplab_ref as ref
from tests.helpers import f16_round
from wsscam import _lib, secdsrg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PRECS = {"f16x3": _lib.PREC_F16X3, "bf16x3": _lib.PREC_BF16X3, "f16": _lib.PREC_F16, "f32": _lib.PREC_F32}


# ---- dilated single layers ------------------------------------------------------------------------------------------------
DIL_SHAPES = [(13, 13, 2), (13, 11, 6), (9, 9, 12), (41, 41, 24), (12, 10, 3)]  # (H, W, dil); N = 2, Cin = 64, 3x3, pad = dil


@functools.lru_cache(maxsize=None)
def _dil_layer(H, W, Cout):
    rng = np.random.default_rng(1000 * H + 10 * W + Cout)
    x = rng.normal(0, 1, (2, 64, H, W)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, 64, 3, 3)) * np.sqrt(2.0 / (64 * 9))).astype(np.float32)
    w *= (1.0 + 0.5 * np.arange(Cout, dtype=np.float32) / Cout)[:, None, None, None]  # (transpose-detecting, as test_gpu_conv.py)
    w *= (1.0 + 0.1 * np.arange(9, dtype=np.float32).reshape(3, 3))[None, None]       # ... and per tap
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    return x, w, shift


def _conv(ctx, x, w, shift, relu, prec, dil, pad, entry="kw"):
    N, Cin, H, W = x.shape
    x_dev = ctx.to_device(x)
    try:
        if entry == "dil":  # wsc_conv2d_nchw_dil itself, whatever the rate
            k = w.shape[2]
            Ho, Wo = H + 2 * pad - ((k - 1) * dil + 1) + 1, W + 2 * pad - ((k - 1) * dil + 1) + 1
            y_dev, shp = ctx.alloc(N * w.shape[0] * Ho * Wo * 4), (N, w.shape[0], Ho, Wo)
            _lib.conv2d_nchw_dil(ctx, x_dev, N, Cin, H, W, w, 1, pad, dil, None, shift, None, relu, prec, y_dev)
        else:
            y_dev, shp = _lib.conv2d_nchw(ctx, x_dev, N, Cin, H, W, w, 1, pad, None, shift, None, relu, prec, dil=dil)
        y = ctx.to_host(y_dev, shp, np.float32)
        y_dev.free()
        return y
    finally:
        x_dev.free()


def _conv_check(y, x, w, shift, relu, prec, dil, pad, what):
    """|y - float64 oracle| within the precision's bound for undilated layers"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    xr, wr = (f16_round(x), f16_round(w)) if prec == _lib.PREC_F16 else (x, w)
    r = F.conv2d(t(xr), t(wr), t(shift), stride=1, padding=pad, dilation=dil)
    A = (F.conv2d(t(x).abs(), t(w).abs(), t(shift).abs(), stride=1, padding=pad, dilation=dil)).numpy()
    if relu:
        r = torch.relu(r)
    r = r.numpy()
    assert y.shape == r.shape, (what, y.shape, r.shape)
    err, mx = np.abs(y.astype(np.float64) - r), np.abs(r).max()
    if prec == _lib.PREC_F16X3:
        bound = np.full_like(r, 4e-6 * mx)
    elif prec == _lib.PREC_BF16X3:
        bound = np.full_like(r, 1e-4 * mx)
    elif prec == _lib.PREC_F16:
        bound = 2.0 ** -11 * np.abs(r) + 3e-4 * mx
    else:
        bound = (x.shape[1] * w.shape[2] * w.shape[3] + 8) * U * A
    print("%s: max err %.3g = %.3g of max|ref| %.3g; worst err / bound %.3g" % (what, err.max(), err.max() / mx, mx, (err / bound).max()))
    assert not (err > bound).any(), "%s: %d beyond the bound, worst err / bound %.3g" % (what, (err > bound).sum(), (err / bound).max())
    return bound


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("shape", DIL_SHAPES, ids=lambda s: "%dx%d-d%d" % s)
def test_dilated_layer_vs_oracle(ctx, shape, prec):
    H, W, dil = shape
    P = PRECS[prec]
    for Cout in (64, 128):
        x, w, shift = _dil_layer(H, W, Cout)
        for relu in (False, True):
            y = _conv(ctx, x, w, shift, relu, P, dil, dil)
            _conv_check(y, x, w, shift, relu, P, dil, dil, "dilated %s Cout %d relu %d %s" % (shape, Cout, relu, prec))
            if dil >= max(H, W):
                # every off-centre tap of every pixel is outside the image: the layer IS the 1x1 layer of its centre tap, run
                # through the same kernel (another K order: the same bound, not the same bits)
                yc = _conv(ctx, x, np.ascontiguousarray(w[:, :, 1:2, 1:2]), shift, relu, P, 1, 0)
                bound = _conv_check(yc, x, w, shift, relu, P, dil, dil, "centre tap of %s Cout %d relu %d %s" % (shape, Cout, relu, prec))
                assert (np.abs(y.astype(np.float64) - yc) <= 2 * bound).all()  # (each within the bound of the one oracle)


@pytest.mark.parametrize("prec", list(PRECS))
def test_dil_one_through_the_new_entry_is_the_old_entry(ctx, prec):
    x, w, shift = _dil_layer(13, 11, 128)
    for relu in (False, True):
        a = _conv(ctx, x, w, shift, relu, PRECS[prec], 1, 1)
        b = _conv(ctx, x, w, shift, relu, PRECS[prec], 1, 1, entry="dil")
        assert np.array_equal(a, b)
    # ... and a 1x1 kernel has no off-centre tap: any rate is rate 1, on the specialised variants too
    w1 = np.ascontiguousarray(w[:, :, :1, :1])
    assert np.array_equal(_conv(ctx, x, w1, shift, True, PRECS[prec], 1, 0), _conv(ctx, x, w1, shift, True, PRECS[prec], 5, 0, entry="dil"))


def test_dilated_layer_does_not_take_the_lds_window(ctx):
    """dil = 2, pad = 2 is a same-size 3x3 / stride 1 f16x3 layer like the ones the LDS input window serves; its address
    arithmetic is for adjacent taps.  Window on and off: the same bits (and the oracle's values, above)."""
    x, w, shift = _dil_layer(13, 13, 64)
    with ctx.option(_lib.OPT_CONV_WINDOW, 1):
        on = _conv(ctx, x, w, shift, True, _lib.PREC_F16X3, 2, 2)
    with ctx.option(_lib.OPT_CONV_WINDOW, 0):
        off = _conv(ctx, x, w, shift, True, _lib.PREC_F16X3, 2, 2)
    assert np.array_equal(on, off)
    _conv_check(on, x, w, shift, True, _lib.PREC_F16X3, 2, 2, "window option, dil 2")


def test_dilation_needs_the_generic_form(ctx):
    x = np.zeros((1, 3, 9, 9), np.float32)
    w = np.zeros((64, 3, 3, 3), np.float32)
    with pytest.raises(_lib.WscError) as ei:
        _conv(ctx, x, w, np.zeros(64, np.float32), False, _lib.PREC_F16X3, 2, 2)
    assert ei.value.status == _lib.WSC_ERR_INVALID


# ---- TF-SAME pools --------------------------------------------------------------------------------------------------------
POOL_SIZES = [(9, 9), (8, 6), (1, 5), (33, 17)]


def _pool(ctx, x, avg, stride, prec):
    N, H, W, C = x.shape
    x_dev = ctx.to_device(x)
    try:
        y_dev, shp = _lib.pool_same_nhwc(ctx, x_dev, N, H, W, C, avg, stride, prec)
        y = ctx.to_host(y_dev, shp, np.float32)
        y_dev.free()
        return y
    finally:
        x_dev.free()


def _split_representable(x):
    """the nearest value an (f16 hi, f16 lo) pair holds"""
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32) + lo.astype(np.float32)


@pytest.mark.parametrize("hw", POOL_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", ["max2", "max1", "avg1"])
def test_pool_same(ctx, hw, mode):
    """Signed inputs: after a ReLU a zero-padded max pool would pass unnoticed."""
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    avg, stride = mode == "avg1", 2 if mode == "max2" else 1
    shape = (2,) + hw + (64,)
    oracle = (lambda a: ref.avg_pool_same(a)) if avg else (lambda a: ref.max_pool_same(a, stride))
    # f16x3: exact on values representable in the planes.  Max returns one of its inputs.  For the average the inputs are
    # multiples of 36 below 2^11 * 36 / 64: every window sum divides by its tap count (2, 3, 4, 6, 9) to an integer <= 1008,
    # which a half holds exactly.
    x3 = (36.0 * rng.integers(-28, 29, shape)).astype(np.float32) if avg else _split_representable(rng.normal(0, 3, shape).astype(np.float32) - 1.0)
    assert np.array_equal(_split_representable(x3), x3)
    y3, r3 = _pool(ctx, x3, avg, stride, _lib.PREC_F16X3), oracle(x3)
    assert y3.shape == r3.shape == (2, -(-hw[0] // stride), -(-hw[1] // stride), 64)
    assert np.array_equal(y3.astype(np.float64), r3)
    if not avg:
        assert (x3 < 0).all(axis=(1, 2)).any() or r3.min() < 0  # (negative maxima exist: zero padding would show)
    # f32: max bit-exact, average within 1 ulp of fp32
    x = (rng.normal(0, 3, shape) - 1.0).astype(np.float32)
    y, r = _pool(ctx, x, avg, stride, _lib.PREC_F32), oracle(x)
    if avg:
        ulp = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
        assert (np.abs(y.astype(np.float64) - r) <= ulp).all(), (np.abs(y - r) / ulp).max()
    else:
        assert np.array_equal(y.astype(np.float64), r) and r.min() < 0
    # the one-plane half mode shares the 16-bit kernel: exact on halves for the maximum
    if not avg:
        xh = x.astype(np.float16).astype(np.float32)
        assert np.array_equal(_pool(ctx, xh, avg, stride, _lib.PREC_F16).astype(np.float64), oracle(xh))


# ---- fc8-softmax ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 6, 21, 29])
@pytest.mark.parametrize("n_in", [1, 4])
def test_fc8_softmax(ctx, C, n_in):
    M, min_prob = 777, 1e-4
    rng = np.random.default_rng(C * 10 + n_in)
    parts = [rng.uniform(-30.0 / n_in, 30.0 / n_in, (M, C)).astype(np.float32) for _ in range(n_in)]
    parts[0][:3] = [[30.0] + [-30.0] * (C - 1), [0.0] * C, [-30.0] * (C - 1) + [29.999]]  # one-hot, uniform, near the spread's ends
    if n_in > 1:
        for p in parts[1:]:
            p[:3] = 0.0
    total = parts[0]
    for p in parts[1:]:
        total = total + p  # float32, in the reference's order fc8_1 + fc8_2 + fc8_3 + fc8_4
    devs = [ctx.to_device(p) for p in parts]
    out = ctx.alloc(2 * M * C * 4)
    try:
        _lib.fc8_softmax(ctx, devs, M, C, out.ptr, min_prob=min_prob, sum_dev=out.ptr + M * C * 4)
        got = ctx.to_host(out, (2, M, C), np.float32)
    finally:
        for d in devs + [out]:
            d.free()
    assert np.array_equal(got[1], total)
    want = ref.fc8_softmax(total, min_prob)
    assert np.abs(got[0].astype(np.float64) - want).max() <= 2e-6
    assert np.abs(got[0].astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    assert got[0].min() >= min_prob / (1 + C * min_prob) * (1 - 1e-6)


# ---- TF bilinear resize --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((41, 41), (321, 321)), ((5, 7), (12, 9)), ((9, 6), (9, 6)), ((321, 300), (41, 41))])
def test_resize_bilinear_tf(ctx, src, dst):
    rng = np.random.default_rng(src[0] + dst[1])
    x = rng.normal(0, 5, (2,) + src + (5,)).astype(np.float32)
    x_dev = ctx.to_device(x)
    y_dev = _lib.resize_bilinear_tf(ctx, x_dev, 2, src[0], src[1], 5, dst[0], dst[1])
    y = ctx.to_host(y_dev, (2,) + dst + (5,), np.float32)
    x_dev.free()
    y_dev.free()
    want = ref.resize_bilinear_tf(x, dst[0], dst[1])
    assert np.abs(y - want).max() <= 1e-6 * np.abs(want).max(), np.abs(y - want).max() / np.abs(want).max()
    if src == dst:
        assert np.array_equal(y, x)


# ---- nets end to end --------------------------------------------------------------------------------------------------------
LOGIT_TOL = {"f16x3": 1e-4, "f32": 2e-5}


@functools.lru_cache(maxsize=None)
def _thin_ref(case):
    wts, x = ref.thin_case(*case)
    fc8, prob = ref.forward(case[0], wts, x)
    return wts, x, fc8, prob


def _net_check(fc8, prob, rfc8, rprob, prec, what):
    mx = np.abs(rfc8).max()
    d, dp = np.abs(fc8 - rfc8).max() / mx, np.abs(prob - rprob).max()
    agree = (fc8.argmax(-1) == rfc8.argmax(-1)).mean()
    print("%s %s: logits %.3g of max|fc8| %.3g (bound %g), softmax %.3g (1e-4), arg-max agreement %.5f" % (what, prec, d, mx, LOGIT_TOL[prec], dp, agree))
    assert fc8.shape == rfc8.shape and prob.shape == rprob.shape
    assert d <= LOGIT_TOL[prec], d
    assert dp <= 1e-4, dp
    assert agree >= ref.ARGMAX_AGREE, agree
    assert np.abs(prob.sum(-1) - 1).max() <= 1e-5


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("case", ref.THIN_CASES, ids=lambda c: "%s-%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1]))
def test_thin_net_vs_oracle(ctx, case, prec):
    wts, x, rfc8, rprob = _thin_ref(case)
    net = secdsrg.SegNet(case[0], wts, case[1], precision=PRECS[prec], ctx=ctx)
    try:
        assert net.map_size(*case[2]) == rfc8.shape[1:3] == (-(-case[2][0] // 8), -(-case[2][1] // 8))
        prob, fc8 = net.forward(x, want_fc8=True)
        _net_check(fc8, prob, rfc8, rprob, prec, "thin %s" % (case,))
        assert np.array_equal(net.softmax(x), prob)
    finally:
        net.close()


@functools.lru_cache(maxsize=None)
def _full_ref():
    wts = ref.random_weights("DSRG", 21, fc_width=1024, seed=11, widths=(64, 128, 256, 512, 512))
    x = ref.net_input(1, 65, 65, 12)
    fc8, prob = ref.forward("DSRG", wts, x)
    return wts, x, fc8, prob


def test_full_width_dsrg_and_the_range_guard(ctx):
    """The real widths once (64 .. 512, fc 1024, 21 classes), He-scaled like a checkpoint; then the same net on an input 1e3
    times larger: f16x3 must report WSC_ERR_RANGE, f32 must compute it."""
    wts, x, rfc8, rprob = _full_ref()
    net = secdsrg.SegNet("DSRG", wts, 21, precision=_lib.PREC_F16X3, ctx=ctx)
    try:
        prob, fc8 = net.forward(x, want_fc8=True)
        _net_check(fc8, prob, rfc8, rprob, "f16x3", "full-width DSRG")
        with pytest.raises(_lib.WscError) as ei:
            net.forward(x * 1e3)
        assert ei.value.status == _lib.WSC_ERR_RANGE
        assert ctx.range_status() == 0  # reported once, scoped to the forward that raised it
        assert np.array_equal(net.forward(x), prob)
    finally:
        net.close()
    net = secdsrg.SegNet("DSRG", wts, 21, precision=_lib.PREC_F32, ctx=ctx)
    try:
        prob, fc8 = net.forward(x, want_fc8=True)
        _net_check(fc8, prob, rfc8, rprob, "f32", "full-width DSRG")
        big = net.forward(x * 1e3, want_fc8=True)[1]
        rbig = ref.forward("DSRG", wts, x * 1e3)[0]
        assert np.isfinite(big).all() and np.abs(big - rbig).max() <= LOGIT_TOL["f32"] * np.abs(rbig).max()
    finally:
        net.close()


# ---- secdsrg.SegNet -----------------------------------------------------------------------------------------------------------
CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)


def test_segnet_round_trip(ctx):
    case = ("DSRG", 5, (65, 65))
    wts, x, rfc8, rprob = _thin_ref(case)
    flat = {}
    for layer, ent in wts.items():
        flat[layer + "_weights"], flat[layer + "_bias"] = ent["w"], ent["b"]
    a, b = secdsrg.SegNet("DSRG", wts, 5, ctx=ctx), secdsrg.SegNet("DSRG", flat, 5, ctx=ctx)
    try:
        prob = a.softmax(x)
        assert np.array_equal(prob, b.softmax(x))  # both weight-dict formats
        assert prob.dtype == np.float32 and prob.shape == (2, 9, 9, 5) and prob.flags["C_CONTIGUOUS"]
        # softmax() feeds the seed growing and the evaluator as it is
        rng = np.random.default_rng(0)
        tags = np.ones((2, 5), np.float32)
        cues = (rng.uniform(size=prob.shape) < 0.05).astype(np.float32)
        grown = secdsrg.generate_seed_step(tags, cues, prob, ctx=ctx)
        assert grown.shape == prob.shape and (grown >= cues).all()
        imgs = [rng.integers(0, 256, (20, 24, 3), dtype=np.uint8) for _ in range(2)]
        gts = [rng.integers(0, 5, (20, 24)).astype(np.uint8) for _ in range(2)]
        ev = secdsrg.SegEvaluator(5, CRF_CFG, ctx=ctx)
        try:
            preds = ev.update(list(prob), imgs, gts, want_pred=True)
            assert preds[0].shape == (20, 24) and 0.0 <= ev.metrics()["mIoU"] <= 1.0
        finally:
            ev.close()
        # create_network's output and pred()'s rescale of it
        out = a.output(x, MEAN, CRF_CFG)
        assert out.shape == (2, 9, 9, 5) and np.allclose(np.exp(out.astype(np.float64)).sum(-1), 1.0, atol=1e-5)
        image = a.resize(x + MEAN.reshape(1, 1, 1, 3), (9, 9))
        assert np.abs(image - ref.resize_bilinear_tf(x + MEAN.reshape(1, 1, 1, 3), 9, 9)).max() <= 1e-6 * 300
        assert np.array_equal(out, secdsrg.crf_layer(prob, image, CRF_CFG, 5, ctx=ctx))
        resc = a.rescale_output(x, MEAN, CRF_CFG)
        assert resc.shape == (2, 65, 65, 5)
        assert np.abs(resc - ref.resize_bilinear_tf(out, 65, 65)).max() <= 1e-6 * np.abs(out).max()
        # image_preprocess: TF resize, RGB -> BGR, minus mean
        pre = a.preprocess(imgs, MEAN, size=(33, 31))
        wantp = np.stack([ref.resize_bilinear_tf(im[None].astype(np.float32), 33, 31)[0][:, :, ::-1] - MEAN for im in imgs])
        assert pre.shape == (2, 33, 31, 3) and np.abs(pre - wantp).max() <= 1e-6 * 255
    finally:
        a.close()
        b.close()
    assert a.net is None
    a.close()  # idempotent


def test_segnet_weight_errors(ctx):
    wts = ref.random_weights("SEC", 5, seed=3)
    init_model = {k: v for k, v in wts.items() if k != "fc8"}  # a pickled init model: fc8 is random in the reference
    with pytest.raises(KeyError, match="fc8"):
        secdsrg.SegNet("SEC", init_model, 5, ctx=ctx)
    with pytest.raises(ValueError):
        secdsrg.SegNet("FCN", wts, 5, ctx=ctx)
    with pytest.raises(ValueError):
        secdsrg.SegNet("SEC", wts, 6, ctx=ctx)  # fc8 has 5 outputs
    # the library itself: WSC_ERR_SHAPE, and the text names the layer
    sd = secdsrg.seg_state_dict("SEC", wts, 5)
    for bad in ({k: v for k, v in sd.items() if k != "conv3_2.b"},
                dict(sd, **{"conv3_2.w": np.ascontiguousarray(np.transpose(sd["conv3_2.w"], (3, 2, 0, 1)))[:, :, :, :3]})):
        with pytest.raises(_lib.WscError) as ei:
            _lib.Net(ctx, _lib.ARCH_DEEPLAB_LFOV, bad, 5, _lib.PREC_F16X3)
        assert ei.value.status == _lib.WSC_ERR_SHAPE and "conv3_2" in str(ei.value)
    # a segmentation net has no CAM head, a CAM entry says so instead of running
    net = _lib.Net(ctx, _lib.ARCH_DEEPLAB_LFOV, sd, 5, _lib.PREC_F16X3)
    try:
        with pytest.raises(_lib.WscError) as ei:
            net.forward_cam(1, 1, 65, 1)
        assert ei.value.status == _lib.WSC_ERR_INVALID
    finally:
        net.close()


def test_segnet_close_after_a_range_error_still_frees(ctx):
    """a cleanup path that goes through the raising wsc_sync frees nothing while the range flag is up."""
    wts, x, _, _ = _thin_ref(("SEC", 5, (65, 65)))
    net = secdsrg.SegNet("SEC", wts, 5, ctx=ctx)
    handle = net.net
    x_dev = ctx.to_device(x * 1e4)
    out = ctx.alloc(2 * 9 * 9 * 5 * 4)
    try:
        handle.forward_seg(x_dev, 2, 65, 65, out)  # the raw entry: the flag is raised and stays up
        with pytest.raises(_lib.WscError) as ei:
            ctx.sync()
        assert ei.value.status == _lib.WSC_ERR_RANGE
        net.close()  # ... with the flag still up
        assert handle.h is None and net.net is None
        assert ctx.range_status(clear=True) != 0
    finally:
        ctx.range_status(clear=True)
        x_dev.free()
        out.free()
    ctx.sync()
