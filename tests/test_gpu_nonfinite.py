"""GPU: a NaN or an inf given to a network-path entry point never comes out as a plausible finite map ("NaN
and inf"; include/wsscam.h, WSC_ERR_RANGE).  Every case asserts the DOCUMENTED outcome of its (entry point, precision):

  L  loud       the call returns WSC_ERR_RANGE with a text that names the cause (a non-finite weight / scale / shift of an IEEE-half
                layer, a non-finite tensor of a state dict), or it raises the ctx's range flag: the sync() directly behind it
                returns WSC_ERR_RANGE and range_status(clear=True) is non-zero
  P  propagate  every cell that is non-finite in the float64 reference is non-finite on the device (NaN where the reference is NaN,
                NaN or the inf of that sign where it is +-inf)

and, in both, that every cell OUTSIDE the poisoned element's cone (tests/nonfinite_ref.py: the cells that read it) is finite and
within the bound the suite already holds for that operation and precision: tests/test_gpu_conv.py (16-bit conv modes),
tests/test_gpu_f32.py (the derived fp32 bound), tests/test_gpu_layers.py / test_gpu_deeplab.py (pools exact; heads), tests/
test_gpu_seg_grad.py (gradient kernels), the SGD steps bit for bit.  The finite control 1e30 must be reported as out of range by
the IEEE-half modes and computed by the modes with fp32's range.  tests/test_nonfinite_oracle.py pins the references on the CPU."""
import functools

import numpy as np
import pytest
import torch

from oracle import cnn_ref, irn_ref
from tests import cls_head_ref, deeplab_grad_ref as gref, deeplab_ref, irn_sgd_ref, layer_ref as lr, nonfinite_ref as nf, seg_sgd_ref
from tests import test_gpu_range
from wsscam import _lib, secdsrg
from wsscam.net import resnet50_cam, resnet50_irn, vgg16_cam

pytestmark = pytest.mark.gpu

NAN = nf.NAN
U = 2.0 ** -24
VALUES = dict(nf.POISONS, control=nf.CONTROL)


def _prec_id(p):
    return lr.PREC_NAME[p]


@pytest.fixture(autouse=True)
def _flag_down_afterwards(request):
    """A case that fails with the shared ctx's sticky flag up must not fail the cases (and the files) behind it"""
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").range_status(clear=True)


def _assert_flag_raised(ctx, what=""):
    """Outcome L through the flag: the sync directly behind the call reports it, it is sticky, and clearing it returns non-zero"""
    with pytest.raises(_lib.WscError) as ei:
        ctx.sync()
    assert ei.value.status == _lib.WSC_ERR_RANGE, (what, ei.value)
    assert ctx.range_status(clear=True) != 0, what
    assert ctx.range_status() == 0
    ctx.sync()


def _assert_refused(fn, word, ctx=None):
    """Outcome L through the status: WSC_ERR_RANGE with a text that names the cause; nothing was flagged"""
    with pytest.raises(_lib.WscError) as ei:
        fn()
    assert ei.value.status == _lib.WSC_ERR_RANGE and word in str(ei.value), ei.value
    if ctx is not None:
        assert ctx.range_status() == 0
        ctx.sync()


# ---- single conv layers -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_ops(shape):
    return nf.conv_operands(shape)


def _conv_device(ctx, ops, shape, use_res, relu, prec):
    N, Cin, H, W, Cout, k, stride, pad = shape
    x_dev = ctx.to_device(ops["x"])
    r_dev = ctx.to_device(ops["residual"]) if use_res else None
    try:
        y_dev, shp = _lib.conv2d_nchw(ctx, x_dev, N, Cin, H, W, ops["w"], stride, pad, ops["scale"], ops["shift"], r_dev, relu, prec)
        return y_dev, shp
    finally:
        x_dev.free()
        if r_dev is not None:
            r_dev.free()


COMBOS = ((False, False), (False, True), (True, False), (True, True))  # (residual, ReLU)


def _check_conv_case(ctx, shape, prec, placement, name, value, use_res, relu, ref_fn):
    what = "%s %s %s=%s res=%d relu=%d" % (shape, lr.PREC_NAME[prec], placement, name, use_res, relu)
    ops = nf.conv_poisoned(_conv_ops(shape), shape, placement, value)
    operand = nf.conv_place(shape, placement)[0]
    # (1e30 is a number to bf16 / bf16x3: the small-Cin input is loud there for NaN / inf only)
    if nf.outcome("conv2d_nchw", prec, operand, shape[1]) == "L" and (prec in nf.HALF_MODES or name != "control"):
        if operand in ("w", "scale", "shift") and name != "control":
            _assert_refused(lambda: _conv_device(ctx, ops, shape, use_res, relu, prec), "not finite", ctx)
            return
        # a poisoned activation (the input pack's flag), or 1e30 anywhere (the pack's flag / the epilogue's saturation)
        y_dev, _ = _conv_device(ctx, ops, shape, use_res, relu, prec)
        y_dev.free()
        _assert_flag_raised(ctx, what)
        return
    y_dev, shp = _conv_device(ctx, ops, shape, use_res, relu, prec)
    y = ctx.to_host(y_dev, shp, np.float32)  # (no range error: these modes raise nothing)
    y_dev.free()
    assert ctx.range_status() == 0
    cone = nf.conv_cone(shape, placement)
    ref, bound = ref_fn(ops, use_res, relu, name, cone)
    if name == "control":
        assert np.isfinite(ref).all()
        nf.assert_outside(y, ref, bound, np.zeros_like(cone), what)  # computed: every cell within the bound
        return
    if nf.nonfinite(ref).any():
        nf.check_placement(cone, ref)
    else:
        assert relu and name in ("pinf", "ninf"), what  # (relu(-inf) = 0 in every cell of the cone: nothing to propagate)
    nf.assert_propagated(y, ref, cone, what)
    nf.assert_outside(y, ref, bound, cone, what)


@pytest.mark.parametrize("placement", nf.CONV_PLACEMENTS)
@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
@pytest.mark.parametrize("shape", nf.CONV_SHAPES, ids=str)
def test_conv_layer_nonfinite(ctx, shape, prec, placement):
    def ref_fn(ops, use_res, relu, name, cone):
        ref = nf.conv_ref(ops, shape, use_res, relu, prec)
        return ref, nf.conv_bound(prec, ref, ops, shape, use_res, cone, _clean_max(shape, prec, use_res, relu))

    for use_res, relu in COMBOS:
        if placement == "residual" and not use_res:
            continue
        for name, value in VALUES.items():
            _check_conv_case(ctx, shape, prec, placement, name, value, use_res, relu, ref_fn)


@functools.lru_cache(maxsize=None)
def _clean_max(shape, prec, use_res, relu):
    """max|ref| of the clean layer: what bounds the cells outside a cone"""
    rounded = prec if prec in (_lib.PREC_BF16, _lib.PREC_F16) else None
    return float(np.abs(nf.conv_ref(_conv_ops(shape), shape, use_res, relu, rounded)).max())


@functools.lru_cache(maxsize=None)
def _big_clean(rounded):
    """CONV_BIG once per operand rounding, fp32 on the CPU (as tests/test_gpu_conv.py at this size): the operands the precision
    holds, the accumulator conv(x, w), conv(|x|, |w|) for the A of the fp32 bound, and the clean pre-activation in float64"""
    shape = nf.CONV_BIG
    ops = dict(_conv_ops(shape))
    if rounded:
        for n in ("x", "w", "residual"):
            ops[n] = nf.bf16_round(ops[n])
    one = {"scale": np.ones_like(ops["scale"]), "shift": np.zeros_like(ops["shift"])}
    raw = nf.conv_ref(dict(ops, **one), shape, False, False, None, dtype=torch.float32)
    A = None
    if not rounded:
        A = nf.conv_ref(dict({k: np.abs(v) for k, v in ops.items()}, **one), shape, False, False, None, dtype=torch.float32)
    pre = raw.astype(np.float64) * ops["scale"].astype(np.float64)[None, :, None, None] + ops["shift"].astype(np.float64)[None, :, None, None] \
        + ops["residual"]
    return ops, raw, A, pre


@pytest.mark.parametrize("name", list(VALUES))
@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
def test_conv_layer_nonfinite_square_tile(ctx, prec, name):
    """The 256 x 256 tile (two 128-row groups), residual and ReLU, every placement with NaN, +-inf and the control.  The clean
    accumulator is the fp32 CPU oracle's (as tests/test_gpu_conv.py at this size); the poisoned reference is computed from it in
    float64 (nonfinite_ref.conv_shifted_ref: the layer is 1 x 1, a cone cell has one changed term).  PREC_F32: the oracle is an
    fp32 chain of the same length, so the bound is twice tests/test_gpu_f32.py's, 2 (K + 8) 2^-24 A, A = conv(|x|, |w|) |scale| +
    |shift| + |residual| of the operands as the case has them (the control's magnitude in its place; a non-finite value left out)."""
    shape = nf.CONV_BIG
    N, Cin, H, W, Cout, k, stride, pad = shape
    ops0, raw, A, pre = _big_clean(prec == _lib.PREC_BF16)
    mx_clean = float(np.maximum(pre, 0).max())
    value = VALUES[name]

    def ref_fn(ops, use_res, relu, name, cone):
        ref = nf.conv_shifted_ref(ops0, raw, shape, ref_fn.placement, value, prec, pre=pre)
        if prec == _lib.PREC_F32:
            op, idx = nf.conv_place(shape, ref_fn.placement)
            mag = abs(value) if np.isfinite(value) else abs(float(ops0[op][idx]))
            Ap = nf.conv_shifted_ref({n: np.abs(v) for n, v in ops0.items()}, A, shape, ref_fn.placement, mag, None)
            return ref, 2 * (Cin * k * k + 8) * U * Ap
        return ref, nf.conv_bound(prec, ref, ops, shape, use_res, cone, mx_clean)

    for placement in nf.CONV_PLACEMENTS:
        ref_fn.placement = placement
        _check_conv_case(ctx, shape, prec, placement, name, value, True, True, ref_fn)


# ---- pools --------------------------------------------------------------------------------------------------------------------
def _pool_run(ctx, entry, x, stride, prec):
    N, H, W, C = x.shape
    x_dev = ctx.to_device(x)
    try:
        if entry == "maxpool":
            return _lib.maxpool_nhwc(ctx, x_dev, N, H, W, C, 3, stride, 1, prec)
        if entry == "tf_same":
            return _lib.pool_tf_nhwc(ctx, x_dev, N, H, W, C, 3, stride, 1, prec)
        return _lib.pool_same_nhwc(ctx, x_dev, N, H, W, C, entry == "same_avg", stride, prec)
    finally:
        x_dev.free()


# (the nets' average pool is 3 x 3 / 1: wsc_pool_same_nhwc takes no other)
POOL_CASES = [(e, g) for e in ("maxpool", "same_max", "same_avg", "tf_same") for g in nf.POOL_GEOMS if e != "same_avg" or g[2] == 1]


@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
@pytest.mark.parametrize("entry,geom", POOL_CASES, ids=lambda v: str(v))
def test_pool_nonfinite(ctx, entry, geom, prec):
    """wsc_maxpool_nhwc, wsc_pool_same_nhwc (max / avg), wsc_pool_tf_nhwc, 3 x 3.  Outside the cone the maximum is exact on the values
    the planes hold (tests/test_gpu_layers.py); the average is the double sum rounded once to fp32 and once to the planes:
    (2^-24 + the planes' half-ulp) |ref| + the half formats' subnormal floor."""
    H, W, stride = geom
    avg, rule = entry == "same_avg", "torch" if entry == "maxpool" else "same"
    rng = np.random.default_rng(H * 100 + W + stride)
    x = (rng.normal(0, 3, (1, H, W, 64)) - 1.0).astype(np.float32)
    for placement in nf.POOL_PLACEMENTS:
        cell = nf.pool_place(H, W, stride, placement)
        cone = nf.pool_cone(H, W, 64, 3, stride, rule, cell)
        for name, value in VALUES.items():
            what = "%s %s %s %s=%s" % (entry, geom, lr.PREC_NAME[prec], placement, name)
            xp = x.copy()
            xp[(0,) + cell] = value
            y_dev, shp = _pool_run(ctx, entry, xp, stride, prec)
            if nf.outcome("pool", prec) == "L":
                y_dev.free()
                _assert_flag_raised(ctx, what)
                continue
            y = ctx.to_host(y_dev, shp, np.float32)
            y_dev.free()
            ref = nf.pool_ref(nf.precision_values(xp, prec), 3, stride, rule, avg)
            bound = (U + lr.HALF_ULP[prec]) * np.where(np.isfinite(ref), np.abs(ref), 0) + lr.ABS_FLOOR[prec] if avg else 0.0
            if name == "control":
                nf.assert_outside(y, ref, bound, np.zeros_like(cone), what)
                continue
            if not nf.nonfinite(ref).any():
                assert name == "ninf"  # (-inf loses every window; the two-plane modes hold it as -inf + NaN: NaN in the cone)
                nf.assert_outside(y, ref, bound, cone, what)
                continue
            nf.check_placement(cone, ref)
            nf.assert_propagated(y, ref, cone, what)
            nf.assert_outside(y, ref, bound, cone, what)


@pytest.mark.parametrize("avg,geom", [(a, g) for a in (False, True) for g in nf.POOL_GEOMS if not a or g[2] == 1], ids=lambda v: str(v))
def test_pool_same_grad_nonfinite(ctx, avg, geom):
    """wsc_pool_same_grad_nhwc (fp32) at 9 x 11 and 13 x 13, stride 2 and 1, a NaN / inf in dy -- of an interior window (at stride 1
    its input cells are shared with the windows around it), of the top right corner window and of the bottom left one, whose
    windows are clamped at the image edge: P over the input cells that receive it; elsewhere tests/test_gpu_seg_grad.py's
    (k k + 2) u sum|terms|."""
    H, W, stride = geom
    rng = np.random.default_rng(17 + stride + H)
    x = rng.normal(0, 1, (1, H, W, 64)).astype(np.float32)
    Ho, Wo = -(-H // stride), -(-W // stride)
    dy0 = rng.normal(0, 1, (1, Ho, Wo, 64)).astype(np.float32)
    xd, dx = ctx.to_device(x), ctx.alloc(x.nbytes)
    try:
        for cell in ((Ho // 2, Wo // 2, 9), (0, Wo - 1, 63), (Ho - 1, 0, 5)):
            for name, value in nf.POISONS.items():
                dy = dy0.copy()
                dy[(0,) + cell] = value
                ref = nf.pool_grad_ref(x, dy, 3, stride, avg)
                cone = nf.pool_grad_cone(x, 3, stride, avg, cell)
                nf.check_placement(cone, ref)
                S = nf.pool_grad_ref(x, np.where(np.isfinite(dy), np.abs(dy), 0), 3, stride, avg)
                gd = ctx.to_device(dy)
                _lib.pool_same_grad_nhwc(ctx, xd, gd, 1, H, W, 64, avg, stride, dx)
                got = ctx.to_host(dx, x.shape, np.float32)
                gd.free()
                what = "%s avg=%d %s=%s" % (geom, avg, cell, name)
                nf.assert_propagated(got, ref, cone, what)
                nf.assert_outside(got, ref, (9 + 2) * U * S, cone, what)
    finally:
        xd.free(), dx.free()


# ---- heads --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
@pytest.mark.parametrize("use_max", [False, True], ids=["mean", "max"])
def test_gap_linear_sigmoid_nonfinite(ctx, use_max, prec):
    """B = 2, hw = 25, F = 64: a poisoned feature of sample 0 is that sample's scores; sample 1 keeps tests/test_gpu_layers.py's
    bound (a quarter of the logit bound + 4 u on the sigmoid)."""
    B, hw, F, C = 2, 25, 64, 5
    rng = np.random.default_rng(9)
    feat = rng.normal(0, 1, (B, hw, F)).astype(np.float32)
    w = rng.normal(0, 0.3, (C, F)).astype(np.float32)
    bias = rng.normal(0, 0.3, C).astype(np.float32)
    cone = np.zeros((B, C), dtype=bool)
    cone[0] = True
    for name, value in VALUES.items():
        what = "%s %s" % (lr.PREC_NAME[prec], name)
        f = feat.copy()
        f[0, 7, 5] = value
        fd = ctx.to_device(f)
        sd, shp = _lib.gap_linear_sigmoid(ctx, fd, B, -hw if use_max else hw, F, w, bias, 1, prec)
        fd.free()
        if nf.outcome("gap_linear_sigmoid", prec) == "L":
            sd.free()
            _assert_flag_raised(ctx, what)
            continue
        score = ctx.to_host(sd, shp, np.float32)
        sd.free()
        v = nf.precision_values(f, prec)
        with np.errstate(over="ignore", invalid="ignore"):
            ref, pooled = lr.gap_linear_sigmoid(v, w, bias, use_max, 1)
        fz = lambda a: np.where(np.isfinite(a), np.abs(a), 0).astype(np.float64)
        gb = np.zeros_like(pooled) if use_max else (-(-hw // 16) + 16) * U * fz(v).mean(1)  # (tests/test_gpu_layers.py's chain)
        aw = np.abs(w.astype(np.float64))
        bound = (gb @ aw.T + (F / 64 + 7) * U * (fz(pooled) @ aw.T)) / 4 + 4 * U
        if name == "control":
            # (1e30 through the Linear: the logit is +-1e29, the sigmoid 0 or 1 -- or, under the mean, nothing but itself)
            nf.assert_outside(score[1:], ref[1:], bound[1:], cone[1:], what)
            assert np.isfinite(score).all() and np.array_equal(score[0], np.where(ref[0] > 0.5, 1.0, 0.0).astype(np.float32))
            continue
        if not nf.nonfinite(ref).any():
            # -inf is never the maximum; an infinite pooled value is a logit of +-inf and a sigmoid of exactly 0 or 1: the reference
            # is finite, nothing to propagate (the two-plane modes hold an inf as inf + NaN: NaN in the cone)
            assert name in ("pinf", "ninf")
            nf.assert_outside(score, ref, bound, cone, what)
            continue
        nf.check_placement(cone, ref)
        nf.assert_propagated(score, ref, cone, what)
        nf.assert_outside(score, ref, bound, cone, what)


def test_cam_flip_add_nonfinite(ctx):
    """relu(head[2b]) + relu(head[2b + 1]).flip: exact outside the cell (tests/test_gpu_layers.py), NaN / +inf in it; relu(-inf) = 0"""
    rng = np.random.default_rng(4)
    head = rng.normal(0, 1, (4, 5, 7, 24)).astype(np.float32)
    for name, value in nf.POISONS.items():
        h = head.copy()
        h[3, 2, 1, 6] = value
        hd = ctx.to_device(h)
        cd, shp = _lib.cam_flip_add(ctx, hd, 2, 5, 7, 20, 24)
        cam = ctx.to_host(cd, shp, np.float32)
        hd.free(), cd.free()
        ref = lr.flip_add(h, 20)
        cone = np.zeros(ref.shape, dtype=bool)
        cone[1, 6, 2, 7 - 1 - 1] = True
        if name == "ninf":
            assert np.isfinite(ref).all() and np.array_equal(cam, ref)
            continue
        nf.check_placement(cone, ref)
        nf.assert_propagated(cam, ref, cone, name)
        assert np.array_equal(cam[~cone], ref[~cone])


def test_fc8_softmax_nonfinite(ctx):
    """M = 50, C = 5: a NaN or +inf logit is its pixel's row of NaN; -inf is probability min_prob / sum (finite, as the reference);
    the other rows keep tests/test_gpu_deeplab.py's 1e-6."""
    M, C = 50, 5
    rng = np.random.default_rng(6)
    z = rng.normal(0, 2, (M, C)).astype(np.float32)
    z[3, 2], z[4, 1], z[5, 0] = NAN, nf.PINF, nf.NINF
    zd, pd = ctx.to_device(z), ctx.alloc(z.nbytes)
    _lib.fc8_softmax(ctx, [zd], M, C, pd, 1e-4)
    p = ctx.to_host(pd, (M, C), np.float32)
    zd.free(), pd.free()
    ref = nf.fc8_softmax_ref(z, 1e-4)
    cone = np.zeros((M, C), dtype=bool)
    cone[3:6] = True
    nf.check_placement(cone, ref)
    nf.assert_propagated(p, ref, cone)
    nf.assert_outside(p, ref, 1e-6, cone)
    assert np.isfinite(p[5]).all() and np.abs(p[5] - ref[5]).max() <= 1e-6


@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
def test_group_norm_nonfinite(ctx, prec):
    """A NaN in x is its (sample, group): P in the modes that hold a NaN, the range flag in the IEEE-half modes (the planes cannot);
    the other groups keep tests/test_gpu_layers.py's bound."""
    N, H, W, C, G = 2, 5, 6, 64, 4
    rng = np.random.default_rng(8)
    x = rng.normal(0, 1, (N, H, W, C)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0, 0.2, C).astype(np.float32)
    x[1, 2, 3, 40] = NAN
    y0 = np.zeros((N, H, W, C), np.float32)
    xd, yd = ctx.to_device(x), ctx.to_device(y0)
    _lib.group_norm_nhwc(ctx, xd, N, H, W, C, gamma, beta, G, 1e-5, 1, True, H, W, C, 0, prec, yd)
    if nf.outcome("group_norm_nhwc", prec) == "L":
        xd.free(), yd.free()
        _assert_flag_raised(ctx)
        return
    y = ctx.to_host(yd, y0.shape, np.float32)
    xd.free(), yd.free()
    ref = lr.group_norm_head(x, gamma, beta, G, 1e-5, 1, True, H, W, y0, 0)
    cone = np.zeros(ref.shape, dtype=bool)
    cone[1, :, :, 32:48] = True
    nf.check_placement(cone, ref)
    nf.assert_propagated(y, ref, cone)
    clean = np.where(cone, 0.0, x)
    mean, rstd, amax = lr.group_stats(clean, G, 1e-5)
    chain = 16 * U * (np.abs(gamma)[None, :] * np.repeat(rstd * (amax + np.abs(mean)), C // G, axis=1) + np.abs(beta)[None, :])
    bound = chain[:, None, None, :] + lr.HALF_ULP[prec] * np.where(cone, 0, np.abs(ref)) + lr.ABS_FLOOR[prec]
    nf.assert_outside(y, ref, bound, cone)


# ---- whole nets: outcome L in every precision -----------------------------------------------------------------------------------
def _cam_model(cls, sd, C, prec):
    return test_gpu_range._model(cls, sd, C, prec)


def _net_input(S=65, seed=13):
    return cnn_ref.msf_pack(cnn_ref.synth_image(np.random.default_rng(seed), 90, 70), (S, S))


def _assert_forward_is_loud(model, x):
    """the forward, or the sync directly behind it, raises WSC_ERR_RANGE; then the flag clears non-zero and a clean forward runs"""
    ctx = model.ctx
    with pytest.raises(_lib.WscError) as ei:
        model.forward(x)
        ctx.sync()
    assert ei.value.status == _lib.WSC_ERR_RANGE, ei.value
    assert ctx.range_status(clear=True) != 0
    ctx.sync()


@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
@pytest.mark.parametrize("case", ["nan_weight", "inf_weight", "nan_running_mean"])
def test_resnet50_cam_nonfinite_checkpoint_is_refused(case, prec):
    """A checkpoint saved after a diverged step: refused when the net is created, in every precision, with the tensor's name"""
    sd = dict(cnn_ref.make_resnet50_cam_state_dict(20, seed=3))
    key = "resnet50.layer1.0.bn2.running_mean" if case == "nan_running_mean" else "resnet50.layer1.0.conv2.weight"
    t = sd[key].clone()
    if case == "nan_running_mean":
        t[5] = NAN
    else:
        t[3, 1, 0, 2] = NAN if case == "nan_weight" else nf.PINF
    sd[key] = t
    x = _net_input()

    def run():
        m = _cam_model(resnet50_cam.CAM, sd, 20, prec)
        m.forward(x)  # (a lazily created net: the first forward creates it)

    _assert_refused(run, key)


@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
def test_resnet50_cam_nan_pixel_is_loud(prec):
    """One NaN input pixel: the reference's CAMs are NaN nearly everywhere; the input pack raises the flag in every precision.
    f16x3: the fused stem + pool kernel and the two-launch form (OPT_STEM_POOL_FUSED) read different packs -- both raise it.
    Then the same ctx gives the clean CAMs of a fresh ctx, bit for bit."""
    sd = cnn_ref.make_resnet50_cam_state_dict(20, seed=3)
    x = _net_input()
    bad = x.copy()
    bad[1, 2, 30, 31] = NAN
    model = _cam_model(resnet50_cam.CAM, sd, 20, prec)
    for fused in ((1, 0) if prec == _lib.PREC_F16X3 else (1,)):
        with model.ctx.option(_lib.OPT_STEM_POOL_FUSED, fused):
            _assert_forward_is_loud(model, bad)
    cam = model.forward(x)
    assert np.isfinite(cam).all() and model.ctx.range_status() == 0
    fresh = _cam_model(resnet50_cam.CAM, sd, 20, prec)
    assert np.array_equal(cam, fresh.forward(x))


@pytest.mark.parametrize("batchnorm", [False, True])
def test_vgg16_cam_nonfinite_is_loud(batchnorm):
    sd = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, 20, batchnorm, seed=6)
    x = _net_input()
    bad = x.copy()
    bad[0, 0, 0, 0] = nf.NINF
    model = _cam_model(vgg16_cam.CAM, sd, 20, _lib.PREC_F16X3)
    _assert_forward_is_loud(model, bad)
    cam, score = model.forward_batch(x[None], want_score=True)
    assert np.isfinite(cam).all() and np.isfinite(score).all()
    first = "vgg16.%s.0.weight" % cnn_ref.VGG16_CFG[0][0]
    sdn = dict(sd)
    sdn[first] = sd[first].clone()
    sdn[first][7, 1, 1, 1] = NAN

    def run():
        _cam_model(vgg16_cam.CAM, sdn, 20, _lib.PREC_F16X3).forward(x)

    _assert_refused(run, first)


@pytest.mark.parametrize("prec", [_lib.PREC_F16X3, _lib.PREC_F32], ids=_prec_id)
@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_thin_deeplab_nan_pixel_is_loud(ctx, method, prec):
    """The thin LFOV / ASPP nets through forward_seg: SegNet.forward reports the flag once, scoped to the forward that raised it
    (tests/test_gpu_deeplab.py), and the next clean forward equals a clean forward before it"""
    wts, x = deeplab_ref.thin_case(method, 5, (65, 65))
    net = secdsrg.SegNet(method, wts, 5, precision=prec, ctx=ctx)
    try:
        clean = net.forward(x)
        bad = x.copy()
        bad[1, 64, 64, 2] = NAN
        with pytest.raises(_lib.WscError) as ei:
            net.forward(bad)
        assert ei.value.status == _lib.WSC_ERR_RANGE
        assert ctx.range_status() == 0
        assert np.array_equal(net.forward(x), clean)
    finally:
        net.close()


def test_resnet50_irn_nan_pixel_is_loud():
    """The ResNet50 IRN edge net at the size of its fixture: L from the forward or the sync behind it"""
    from tests import test_gpu_irn

    g = np.load(test_gpu_irn.GOLDEN)
    sd = irn_ref.make_resnet50_irn_state_dict(seed=int(g["seed"]))
    m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=int(g["crop_size"]), stride=int(g["stride"]), precision=_lib.PREC_F16X3)
    m.load_state_dict(sd)
    m.eval().cuda(0)
    x = np.array(g["x"], dtype=np.float32)
    bad = x.copy()
    bad[(0,) * (bad.ndim - 1) + (3,)] = NAN
    _assert_forward_is_loud(m, bad)
    edge, dp = m.forward(x)
    assert np.isfinite(edge).all() and np.isfinite(dp).all()


# ---- the classifier loss and the gradient kernels: P ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mean", "max"])
def test_cls_loss_nonfinite(ctx, kind):
    """B = 2, n = 9, F = 64, C = 5.  A NaN feature of sample 0: both losses NaN, that sample's scores and every weight / bias
    gradient NaN, sample 1's scores and feature gradient at tests/test_gpu_cls_head.py's bound.  A NaN Dense weight: its class."""
    from tests import test_gpu_cls_head as tch

    feat, w, bias, target, _ = cls_head_ref.make_case((2, 9, 64, 5), kind, with_weights=False)
    f = feat.copy()
    f[0, 4, 10] = NAN
    got, ref = tch.run(ctx, kind, f, w, bias, target, None), cls_head_ref.cls_loss(f, kind, w, bias, target)
    assert np.isnan(got["loss"][0]) and np.isnan(got["loss"][1]) and np.isnan(ref["values"]["loss"])
    for key, rk in (("score", "p"), ("feat", "g_feat"), ("w", "g_w"), ("bias", "g_bias")):
        r = ref[rk]
        cone = nf.nonfinite(r)
        assert cone.any()
        nf.assert_propagated(got[key], r, cone, key)
        if (~cone).any():
            assert tch.excess(got[key][~cone], r[~cone])[0] <= 0, key
    assert np.isfinite(got["score"][1]).all() and np.isfinite(got["feat"][1]).all()
    # the counts leave a NaN score out (it has no rounding) and count the other cells as ever
    for slot, key in zip(_lib.CLS_LOSS_SLOTS[2:], ("n_equal", "tp", "possible", "predicted")):
        assert slot == key and got["loss"][2 + _lib.CLS_LOSS_SLOTS[2:].index(slot)] == ref["values"][key], (key, got["loss"], ref["values"])
    wn = w.copy()
    wn[2, 7] = NAN
    got, ref = tch.run(ctx, kind, feat, wn, bias, target, None), cls_head_ref.cls_loss(feat, kind, wn, bias, target)
    assert np.isnan(got["loss"][0])
    for key, rk in (("score", "p"), ("w", "g_w"), ("bias", "g_bias")):
        cone = nf.nonfinite(ref[rk])
        assert cone.any() and (~cone).any()
        nf.assert_propagated(got[key], ref[rk], cone, key)
        assert np.isfinite(got[key][~cone]).all() and tch.excess(got[key][~cone], ref[rk][~cone])[0] <= 0, key
    assert np.isnan(got["feat"]).any()  # (the class's gradient reaches the features through its weights)


@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_seg_loss_nan_probability(ctx, method):
    """wsc_seg_loss at its test file's smallest non-degenerate size: one NaN probability is a NaN `norm` (the constrain term reads
    every probability; SEC's rank sort keys carry the pixel index beside the value, so no position comes from a value)"""
    from tests import seg_loss_ref, test_gpu_seg_loss as tsl

    prob, crf, cues, labels = seg_loss_ref.make_case((3, 7, 5, 5))
    p = prob.copy()
    p[0, 3, 2, 1] = NAN
    loss, g_p, g_z = tsl.run(ctx, method, p, crf, cues, labels)
    got = dict(zip(seg_loss_ref.KEYS, loss))
    assert np.isnan(got["norm"]) and np.isnan(got["constrain"]), got
    assert np.isnan(g_p[0, 3, 2, 1]) and np.isfinite(g_p[1:]).all()  # (the other images' gradients do not read it)
    assert ctx.range_status() == 0


def test_irn_aff_loss_nan_inputs(ctx):
    """wsc_irn_aff_loss: a NaN edge logit is the maximum of every path through it (torch's max carries it), so `total` is NaN; a
    NaN displacement is a NaN `total` through the pairs that read it"""
    from tests import irn_loss_ref, test_gpu_irn_loss as til

    case = irn_loss_ref.CASES[1]
    edge, dp, label = irn_loss_ref.make_case(case)
    e, d = edge.copy(), dp.copy()
    e[0, 4, 5] = NAN
    d[1, 0, 4, 5] = NAN
    for ee, dd, keys in ((e, dp, ("total", "pos", "neg")), (edge, d, ("total",))):
        want = irn_loss_ref.tensor_form(ee, dd, label, case[0], grad=False)["loss"]
        loss, _, _ = til.run(ctx, ee, dd, label, case[0])
        got = dict(zip(irn_loss_ref.KEYS, loss[:len(irn_loss_ref.KEYS)]))
        for k in keys:
            assert np.isnan(want[k]) and np.isnan(got[k]), (k, want[k], got[k])
        assert got["n_bg"] == want["n_bg"] and got["n_fg"] == want["n_fg"] and got["n_neg"] == want["n_neg"]


def test_gradient_kernels_nan_in_dy(ctx):
    """N = 1, 9 x 9, 64 -> 64, k = 3, one NaN in dy: wsc_relu_bias_grad(_scaled) (dz that cell, db its column), wsc_conv2d_wgrad_nhwc
    (dw, db of that output channel), wsc_conv2d_dgrad_nhwc (the 3 x 3 input pixels around it, every channel); the bounds of
    tests/test_gpu_seg_grad.py elsewhere."""
    N, H, W, Cin, Cout, k = 1, 9, 9, 64, 64, 3
    rng = np.random.default_rng(21)
    x = np.maximum(rng.standard_normal((N, H, W, Cin)), -0.5).astype(np.float32)
    y = np.maximum(rng.standard_normal((N, H, W, Cout)), 0).astype(np.float32)
    dy = (1e-3 * rng.standard_normal((N, H, W, Cout))).astype(np.float32)
    wt = rng.standard_normal((k, k, Cin, Cout)).astype(np.float32)
    y[0, 4, 5, 3] = 1.0
    dy[0, 4, 5, 3] = NAN
    M = N * H * W
    xd, yd, gd = ctx.to_device(x), ctx.to_device(y), ctx.to_device(dy)
    dz_d, db_d, dw_d, dx_d = ctx.alloc(dy.nbytes), ctx.alloc(4 * Cout), ctx.alloc(wt.nbytes), ctx.alloc(x.nbytes)
    try:
        for scale in (None, 2.0):
            if scale is None:
                _lib.relu_bias_grad(ctx, yd, gd, M, Cout, dz_d, db_d)
            else:
                _lib.relu_bias_grad_scaled(ctx, yd, gd, M, Cout, scale, dz_d, db_d)
            dz, db = ctx.to_host(dz_d, (M, Cout), np.float32), ctx.to_host(db_d, (Cout,), np.float32)
            rz, rb = nf.relu_bias_grad_ref(y.reshape(M, Cout), dy.reshape(M, Cout), scale or 1.0)
            assert np.isnan(dz[4 * W + 5, 3]) and np.isnan(dz).sum() == 1 and np.isnan(db[3]) and np.isnan(db).sum() == 1
            keep = np.isfinite(rz)
            assert np.array_equal(dz[keep].astype(np.float64), rz[keep].astype(np.float32).astype(np.float64))
            fin = np.isfinite(rb)
            assert (np.abs(db[fin] - rb[fin]) <= (M + 2) * U * np.abs(np.where(keep, rz, 0)).sum(0)[fin]).all()
        _lib.conv2d_wgrad_nhwc(ctx, xd, gd, N, H, W, Cin, Cout, k, 1, 0, dw_d, db_d)
        dw, db = ctx.to_host(dw_d, wt.shape, np.float32), ctx.to_host(db_d, (Cout,), np.float32)
        with np.errstate(invalid="ignore"):
            dw64, db64, S, n, Sb = gref.wgrad_ref(x, dy, k, 1)
        cone = np.zeros(wt.shape, dtype=bool)
        cone[:, :, :, 3] = True
        nf.check_placement(cone, dw64)
        nf.assert_propagated(dw, dw64, cone, "dw")
        nf.assert_outside(dw, dw64, (n[:, :, None, None] + 2) * U * np.where(cone, 0, S), cone, "dw")
        assert np.isnan(db[3]) and np.isnan(db64[3]) and (np.abs(np.delete(db - db64, 3)) <= (M + 2) * U * np.delete(Sb, 3)).all()
        _lib.conv2d_dgrad_nhwc(ctx, gd, wt, N, H, W, Cin, Cout, k, 1, dx_d)
        dx = ctx.to_host(dx_d, x.shape, np.float32)
        with np.errstate(invalid="ignore"):
            dx64, S = gref.dgrad_ref(dy, wt, 1)
        cone = np.zeros(x.shape, dtype=bool)
        cone[0, 3:6, 4:7, :] = True
        nf.check_placement(cone, dx64)
        nf.assert_propagated(dx, dx64, cone, "dx")
        nf.assert_outside(dx, dx64, (k * k * Cout + 2) * U * np.where(cone, 0, S), cone, "dx")
    finally:
        for d in (xd, yd, gd, dz_d, db_d, dw_d, dx_d):
            d.free()


# ---- optimisers and the device repack -------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _one_element(clean, got, at, what):
    assert not np.isfinite(got[at]), (what, got[at])
    assert np.array_equal(np.delete(_bits(got), at), np.delete(_bits(clean), at)), what


@pytest.mark.parametrize("name", list(nf.POISONS))
def test_seg_sgd_nonfinite_gradient(ctx, name):
    """wsc_seg_sgd_accumulate / _apply on the thin DSRG layout: one poisoned gradient element is that element of the accumulator,
    the momentum and the parameter; every other element has the clean run's bits (tests/seg_sgd_ref.py, float32)."""
    weights = deeplab_ref.random_weights("DSRG", 5, 64, 128, seed=8)
    net = secdsrg.SegNet("DSRG", weights, 5, precision=_lib.PREC_F32, ctx=ctx)
    try:
        sg = net._ensure_grad()
        layout, n = seg_sgd_ref.layout_of("DSRG", weights)
        segs = seg_sgd_ref.segments(layout)
        rng = np.random.default_rng(31)
        p, acc, mom = (rng.standard_normal(n).astype(np.float32) * s for s in (1.0, 1e-3, 1e-2))
        g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        for at in (segs[0][1] + 5, segs[-1][2] - 1):  # a weight of the first layer, the last bias
            gp = g.copy()
            gp[at] = nf.POISONS[name]
            out = {}
            for tag, grad in (("clean", g), ("bad", gp)):
                pd, gd, ad, md = (ctx.to_device(a) for a in (p, grad, acc, mom))
                sg.sgd_accumulate(pd, gd, ad, 5e-4, 1)
                sg.sgd_apply(pd, ad, md, np.float32(1e-4), np.float32(0.9), False)
                out[tag] = [ctx.to_host(d, (n,), np.float32) for d in (pd, ad, md)]
                for d in (pd, gd, ad, md):
                    d.free()
            aw = seg_sgd_ref.accumulate(segs, p, g, acc, 5e-4, 1)
            pw, _, mw = seg_sgd_ref.apply(p, aw, mom, 1e-4, 0.9, False)
            for what, clean, got, want in zip(("param", "accum", "mom"), out["clean"], out["bad"], (pw, aw, mw)):
                assert np.array_equal(_bits(clean), _bits(want)), what
                _one_element(clean, got, at, what)
        assert ctx.range_status() == 0
    finally:
        net.close()


@pytest.mark.parametrize("name", list(nf.POISONS))
def test_irn_sgd_nonfinite_gradient(name):
    """wsc_irn_sgd_step on the M7 IRNet layout: the poisoned gradient element is that element of the momentum and the parameter;
    every other element has the bits of the clean step (tests/irn_sgd_ref.py, float32)."""
    from tests import test_gpu_irn_sgd as tis

    sd = tis.base_sd("m7")
    m = tis.fresh_model("m7", sd)
    ctx, grad = m.ctx, m.irn_grad()
    n, b = grad.grad_elems, irn_sgd_ref.boundary(sd, "m7")
    p, g = tis._step_data(n, b)
    mom = (1e-2 * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
    pw, mw = irn_sgd_ref.sgd_step32(p, g, mom, b, 0.1, 1.0, 1e-4, 0.9)
    for at in (b - 1, n - 1):  # the last element at the edge rate, the last at the dp rate
        gp = g.copy()
        gp[at] = nf.POISONS[name]
        out = {}
        for tag, gg in (("clean", g), ("bad", gp)):
            pd, gd, md = ctx.to_device(p), ctx.to_device(gg), ctx.to_device(mom)
            grad.sgd_step(pd, gd, md, 0.1, 1.0, 1e-4, 0.9)
            out[tag] = [ctx.to_host(d, (n,), np.float32) for d in (pd, md)]
            for d in (pd, gd, md):
                d.free()
        for what, clean, got, want in zip(("param", "mom"), out["clean"], out["bad"], (pw, mw)):
            assert np.array_equal(_bits(clean), _bits(want)), what
            _one_element(clean, got, at, what)
    assert ctx.range_status() == 0


def test_irn_load_params_nonfinite_is_loud():
    """wsc_net_irn_load_params with a NaN conv weight / an inf GroupNorm parameter: L at the load (the repack and the vector copy
    raise the flag); the clean parameters load clean afterwards."""
    from tests import test_gpu_irn_sgd as tis

    sd = tis.base_sd("m7")
    m = tis.fresh_model("m7", sd)
    ctx, grad = m.ctx, m.irn_grad()
    flat = irn_sgd_ref.flat_params(sd, "m7")
    conv = next(e for e in grad.layout if e["conv"])
    vec = next(e for e in grad.layout if not e["conv"])
    for at, value in ((conv["offset"] + 3, NAN), (vec["offset"] + 1, nf.PINF)):
        bad = flat.copy()
        bad[at] = value
        pd = ctx.to_device(bad)
        grad.load_params(pd)
        _assert_flag_raised(ctx, str(at))
        pd.free()
    pd = ctx.to_device(flat)
    grad.load_params(pd)
    ctx.sync()
    pd.free()
    assert ctx.range_status() == 0


def test_seg_load_params_nonfinite_is_loud(ctx):
    """wsc_net_seg_load_params with one NaN / inf parameter (a weight of a generic layer, of the first layer, a bias): the repack
    raises the range flag -- L at the load, reported by the sync behind it, in every precision; the clean parameters loaded
    afterwards give the clean forward bit for bit."""
    weights, x = deeplab_ref.thin_case("DSRG", 5, (65, 65))
    for prec in (_lib.PREC_F16X3, _lib.PREC_F32, _lib.PREC_BF16X3):
        net = secdsrg.SegNet("DSRG", weights, 5, precision=prec, ctx=ctx)
        try:
            clean = net.forward(x)
            sg = net._ensure_grad()
            layout, n = seg_sgd_ref.layout_of("DSRG", weights)
            flat = net.flat_params(weights)
            first, some = list(layout.values())[0], list(layout.values())[3]
            for at, value in ((some["w_off"] + 77, NAN), (first["w_off"] + 5, nf.PINF), (some["b_off"] + 1, nf.NINF)):
                bad = flat.copy()
                bad[at] = value
                pd = ctx.to_device(bad)
                sg.load_params(pd)
                _assert_flag_raised(ctx, "%s %d" % (lr.PREC_NAME[prec], at))
                pd.free()
            pd = ctx.to_device(flat)
            sg.load_params(pd)
            ctx.sync()
            pd.free()
            assert ctx.range_status() == 0 and np.array_equal(net.forward(x), clean)
        finally:
            net.close()


def test_seg_trainer_refuses_a_nonfinite_checkpoint(ctx):
    """SegTrainer on a thin DSRG net whose parameters hold one NaN (a checkpoint saved after a diverged step): L when the trainer
    creates its net, before any step runs; the ctx stays clean and a trainer on the clean weights is created behind it."""
    weights, _ = deeplab_ref.thin_case("DSRG", 5, (65, 65))
    bad = {k: dict(v) for k, v in weights.items()}
    bad["conv3_2"]["w"] = np.array(weights["conv3_2"]["w"], dtype=np.float32)
    bad["conv3_2"]["w"][1, 2, 3, 4] = NAN
    _assert_refused(lambda: secdsrg.SegTrainer("DSRG", bad, 5, ctx=ctx), "non-finite", ctx)
    secdsrg.SegTrainer("DSRG", weights, 5, ctx=ctx).close()


def _poison_resident(ctx, tr, at):
    """one NaN into the trainer's resident parameter buffer, behind the net's back: the packed weights stay clean"""
    flat = tr.params.to_host().reshape(-1)
    flat[at] = NAN
    tr.params.free()
    tr.params = None
    tr.params = secdsrg.DeviceMaps.from_host(ctx, flat)


def test_seg_trainer_step_with_a_nan_parameter(ctx):
    """SegTrainer.step on the thin DSRG net with one NaN in the resident parameters (what a diverged update leaves).  The forward,
    the CRF and the region growing run on the net's clean packed weights; the weight-decay term makes that element of the
    accumulator NaN, the update writes it, the repack raises the flag and the step raises WSC_ERR_RANGE at its one download.
    Afterwards, as DESIGN.md 5.1 documents: `calls` counts the step, the update is applied -- every other element of the
    parameters and the momentum has the clean step's bits, the accumulator is cleared -- and the flag is up until cleared."""
    from tests import test_gpu_seg_sgd as tss

    weights, x, cues, tags = tss._step_case("DSRG")
    layout, n = seg_sgd_ref.layout_of("DSRG", weights)
    at = layout["conv3_2"]["w_off"] + 77
    out = {}
    for tag in ("clean", "bad"):
        tr = secdsrg.SegTrainer("DSRG", weights, 5, ctx=ctx)
        try:
            if tag == "bad":
                _poison_resident(ctx, tr, at)
                with pytest.raises(_lib.WscError) as ei:
                    tr.step(x, cues, tags, tss.MEAN, tss.CRF_CFG, epoch=0)
                assert ei.value.status == _lib.WSC_ERR_RANGE, ei.value
                assert ctx.range_status(clear=True) != 0 and ctx.range_status() == 0
            else:
                losses, new_cues = tr.step(x, cues, tags, tss.MEAN, tss.CRF_CFG, epoch=0)
                new_cues.free()
                assert np.isfinite(losses["total"])
            out[tag] = (tr.calls, tr.params.to_host().reshape(-1), tr.mom.to_host().reshape(-1), tr.accum.to_host().reshape(-1))
        finally:
            tr.close()
    assert out["clean"][0] == out["bad"][0] == 1
    _one_element(out["clean"][1], out["bad"][1], at, "param")
    _one_element(out["clean"][2], out["bad"][2], at, "mom")
    assert not out["bad"][3].any() and not out["clean"][3].any()


def test_irn_trainer_step_with_a_nan_parameter(ctx):
    """IrnTrainer.step with one NaN in the resident parameters: the step downloads only the losses (taken on the net's clean
    packed heads: the clean step's values) and returns; the update writes the NaN, the repack raises the flag, and the sync
    behind the step reports it.  Afterwards: global_step counts the step, every other element of the parameters and the
    momentum has the clean step's bits, the flag is up until cleared."""
    from tests import test_gpu_irn_sgd as tis
    from wsscam import irn_train

    sd0 = tis.base_sd("vgg16")
    x, label = tis._trainer_case()
    out = {}
    for tag in ("clean", "bad"):
        m = tis.fresh_model("vgg16", sd0, ctx=ctx)
        tr = irn_train.IrnTrainer(m, tis.PathIndex(5), tis.LR, tis.WD, tis.MAX_STEP, power=tis.POWER)
        try:
            if tag == "bad":
                at = next(e for e in tr.grad.layout if e["conv"])["offset"] + 3
                _poison_resident(ctx, tr, at)
            losses = tr.step(x, label)
            if tag == "bad":
                _assert_flag_raised(ctx, "IrnTrainer.step")
            else:
                ctx.sync()
            out[tag] = (tr.global_step, losses, tr.params.to_host().reshape(-1), tr.mom.to_host().reshape(-1))
        finally:
            tr.close()
            m._release_net()
    assert out["clean"][0] == out["bad"][0] == 1 and out["clean"][1] == out["bad"][1] and np.isfinite(out["bad"][1]["total"])
    _one_element(out["clean"][2], out["bad"][2], at, "param")
    _one_element(out["clean"][3], out["bad"][3], at, "mom")


# ---- recovery and the release paths ---------------------------------------------------------------------------------------------
def test_release_paths_after_a_range_error():
    """After an uncleared range error Net.close() still reaches wsc_net_destroy (it does not raise, and models of the same size can
    be created again and again on the ctx), Context.to_device() returns its buffer, and the error is still there for the next sync()."""
    ctx = _lib.Context(0)
    try:
        sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=3).items()}
        x = _net_input()
        bad = x.copy()
        bad[0, 0, 5, 5] = NAN
        for _ in range(3):
            net = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, sd, 20, _lib.PREC_F16X3)
            hh = net.cam_size(65)
            cd = ctx.alloc(20 * hh * hh * 4)
            xd = ctx.to_device(bad)
            net.forward_cam(xd, 1, 65, cd)
            with pytest.raises(_lib.WscError):
                ctx.sync()
            buf = ctx.to_device(np.arange(16, dtype=np.float32))  # the flag is up: the upload completes and the buffer comes back
            assert buf.ptr
            buf.free()
            net.close()  # (raised before the fix, and left the weights allocated)
            assert net.h is None
            with pytest.raises(_lib.WscError) as ei:  # the error was not swallowed by the release paths
                ctx.sync()
            assert ei.value.status == _lib.WSC_ERR_RANGE
            assert ctx.range_status(clear=True) != 0
            xd.free(), cd.free()
        ctx.sync()
    finally:
        ctx.close()
