"""GPU: the backward pass of the SEC / DSRG DeepLab-VGG16 net (csrc/seg_grad.hip, the pool gradients of csrc/pool.hip,
wsc_net_forward_seg_tape / wsc_net_backward_seg of csrc/net.hip; secdsrg.SegNet.backward_dev / grad_step_dev) against the float64
oracle tests/deeplab_grad_ref.py.

u = 2^-24 throughout.  The per-op tests compare with float64 on the identical float32 operands, elementwise, with bounds that hold
for any summation order:
  weight gradient  |d| <= (n + 2) u sum|x||dz|, n the number of in-image terms of that element (a tap with none: exactly 0.0);
                   db: (n + 2) u sum|dz|; a repeated call gives identical bits
  data gradient    (k k Cout + 2) u sum|dz||w|, random asymmetric kernels: a wrong rotation or transpose is an O(1) error
  mask + bias      dz bit-exact (dy or +0.0)
  pool gradients   (k k + 2) u sum|terms|; with dy of small integers the max-pool result is exact
The end-to-end test runs wsc_net_backward_seg on the device's own tape against chain_grads(float64) on that same downloaded
tape: per layer max|d| <= 64 R32_CHAIN max|g64| for w and for b.  It guards the wiring (a wrong layer, mask, rotation, branch
sum, pool geometry: the smallest such error seen, one flipped decision, is 2.6e-2); the arithmetic is held by the per-op bounds.
Every test prints the figure it asserts on.

Every device output of a per-op test (dw, db, dx, dz) has GUARD floats of CANARY behind it that must survive the call, and its own
region must be overwritten entirely; the full-width network test does the same with the gradient buffer.  The *_FULL cases are
the real layer widths (64 ... 512, fc 1024, 21 classes) on maps of a few pixels, the *_SMALL cases the degenerate maps (H = 1,
W = 1, fewer pixels than a K-step, more K slices than K-steps)."""
import functools

import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import deeplab_grad_ref as gref
from tests import deeplab_ref as ref
from wsscam import _lib, secdsrg
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
CANARY = np.float32(-777.25)
GUARD = 256  # floats of CANARY behind every device output


def _id(s):
    return "x".join(str(v) for v in s)


def _guarded(ctx, shape):
    """a device buffer of prod(shape) + GUARD floats, every one CANARY"""
    return DeviceMaps.from_host(ctx, np.full((int(np.prod(shape)) + GUARD,), CANARY, np.float32))


def _checked(buf, shape, what):
    """the output of a _guarded buffer: the guard band behind it untouched, the output itself overwritten everywhere"""
    flat = buf.to_host()
    n = int(np.prod(shape))
    assert flat.size == n + GUARD
    assert np.array_equal(flat[n:].view(np.uint32), np.full((GUARD,), CANARY, np.float32).view(np.uint32)), what + ": a store behind the output"
    assert not (flat[:n] == CANARY).any(), what + ": an element was not written"
    return flat[:n].reshape(shape).copy()


def _relu_like(rng, shape):
    """post-ReLU-like: half zeros, the positives multiples of 1/4 (equal maxima occur among positive values)"""
    return (np.maximum(rng.integers(-8, 9, shape), 0) / 4.0).astype(np.float32)


# ---- weight gradient ----------------------------------------------------------------------------------------------------------
WGRAD_CASES = [(2, 7, 5, 64, 64, 3, 1, 0), (1, 9, 9, 64, 128, 3, 2, 1), (2, 9, 9, 128, 64, 3, 6, 0), (1, 9, 9, 64, 64, 3, 12, 0),
               (3, 33, 31, 64, 192, 3, 1, 1), (3, 33, 31, 64, 192, 3, 1, 2), (3, 33, 31, 64, 192, 3, 1, 5),
               (2, 13, 11, 3, 64, 3, 1, 0), (2, 13, 11, 3, 128, 3, 1, 0), (2, 8, 6, 128, 21, 1, 1, 0), (2, 8, 6, 128, 5, 1, 1, 0), (2, 8, 6, 64, 128, 1, 1, 0)]
# the real widths: SEC fc6 (centre tap only), DSRG fc6_1 (nine live taps, 576 tiles), fc7, fc8 (16 row tiles x the 32-column
# register-staged tile), conv4_1, conv5_x, conv3_1
WGRAD_FULL_CASES = [(1, 9, 9, 512, 1024, 3, 12, 0), (1, 9, 9, 512, 1024, 3, 6, 0), (1, 5, 7, 1024, 1024, 1, 1, 0), (2, 5, 7, 1024, 21, 1, 1, 0),
                    (1, 9, 9, 256, 512, 3, 1, 2), (1, 9, 9, 512, 512, 3, 2, 0), (1, 17, 17, 128, 256, 3, 1, 3)]
# M = 1; 7 slices asked of 1 K-step; H = 1; W = 1; M = 32 (exactly one K-step); M = 64 in two slices of one K-step; the Cin = 3
# form at M = 4; the smallest Cout; a full 32-column tile; 256 slices asked of 96 K-steps
WGRAD_SMALL_CASES = [(1, 1, 1, 64, 64, 3, 1, 0), (1, 1, 1, 64, 64, 1, 1, 7), (1, 1, 7, 64, 64, 3, 1, 0), (2, 7, 1, 64, 128, 3, 1, 0),
                     (2, 4, 4, 64, 64, 3, 1, 0), (1, 8, 8, 64, 64, 3, 2, 2), (1, 2, 2, 3, 64, 3, 1, 0), (2, 5, 3, 64, 2, 1, 1, 0),
                     (2, 5, 3, 64, 32, 1, 1, 0), (3, 33, 31, 64, 192, 3, 1, 256)]
# (case without its split count) -> the taps that have an in-image term for some pixel
WGRAD_LIVE_TAPS = {(1, 1, 1, 64, 64, 3, 1): [[0, 0, 0], [0, 1, 0], [0, 0, 0]], (1, 1, 7, 64, 64, 3, 1): [[0, 0, 0], [1, 1, 1], [0, 0, 0]],
                   (2, 7, 1, 64, 128, 3, 1): [[0, 1, 0], [0, 1, 0], [0, 1, 0]], (1, 9, 9, 512, 1024, 3, 12): [[0, 0, 0], [0, 1, 0], [0, 0, 0]],
                   (1, 9, 9, 512, 1024, 3, 6): [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}
# a split count above the K-step count is clamped to it: (case) -> the K-steps of its pixels, ceil(M / 32)
WGRAD_CLAMPED = {(1, 1, 1, 64, 64, 1, 1, 7): 1, (3, 33, 31, 64, 192, 3, 1, 256): 96}


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape):
    """(x, dz, the oracle's tuple) of a case without its split count: computed once, shared, never modified"""
    N, H, W, Cin, Cout, k, dil = shape
    rng = np.random.default_rng(sum(shape))
    x = np.maximum(rng.standard_normal((N, H, W, Cin)), -0.5).astype(np.float32)
    dz = (1e-3 * rng.standard_normal((N, H, W, Cout))).astype(np.float32)
    return x, dz, gref.wgrad_ref(x, dz, k, dil)


def _run_wgrad(ctx, x, dz, shape, splits):
    N, H, W, Cin, Cout, k, dil = shape
    with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, dz) as zd, _guarded(ctx, (k, k, Cin, Cout)) as dw, \
            _guarded(ctx, (Cout,)) as db:
        _lib.conv2d_wgrad_nhwc(ctx, xd.ptr, zd.ptr, N, H, W, Cin, Cout, k, dil, splits, dw.ptr, db.ptr)
        return _checked(dw, (k, k, Cin, Cout), "dw"), _checked(db, (Cout,), "db")


@pytest.mark.parametrize("case", WGRAD_CASES + WGRAD_FULL_CASES + WGRAD_SMALL_CASES, ids=_id)
def test_wgrad(ctx, case):
    shape, splits = case[:7], case[7]
    k = shape[5]
    x, dz, (dw64, db64, S, n, Sb) = _wgrad_case(shape)
    dw, db = _run_wgrad(ctx, x, dz, shape, splits)
    bound = (n[:, :, None, None] + 2) * U * S
    err = np.abs(dw.astype(np.float64) - dw64)
    print("wgrad %s: max err / bound %.3f, max err %.3e, max|dW| %.3e" % (_id(case), float((err / np.maximum(bound, 1e-300)).max()),
                                                                         err.max(), np.abs(dw64).max()))
    assert (err <= bound).all()
    for r in range(k):
        for s in range(k):
            if n[r, s] == 0:  # a tap outside the image for every pixel: exact zeros (+0.0)
                assert not dw[r, s].any() and not np.signbit(dw[r, s]).any()
    M = x.shape[0] * x.shape[1] * x.shape[2]
    errb = np.abs(db.astype(np.float64) - db64)
    print("       db: max err / bound %.3f" % float((errb / ((M + 2) * U * Sb)).max()))
    assert (errb <= (M + 2) * U * Sb).all()
    dw2, db2 = _run_wgrad(ctx, x, dz, shape, splits)  # a second call: the same bits
    assert np.array_equal(dw.view(np.uint32), dw2.view(np.uint32)) and np.array_equal(db.view(np.uint32), db2.view(np.uint32))
    if shape in WGRAD_LIVE_TAPS:  # the oracle's count of in-image terms has the pattern, and with it (above) the device's zeros
        assert (n > 0).astype(int).tolist() == WGRAD_LIVE_TAPS[shape]
        assert all(dw[r, s].any() for r in range(k) for s in range(k) if n[r, s] > 0)
    if case in WGRAD_CLAMPED:  # more slices than K-steps: the bits of one slice per K-step
        assert WGRAD_CLAMPED[case] == -(-M // 32) < splits
        dw3, db3 = _run_wgrad(ctx, x, dz, shape, WGRAD_CLAMPED[case])
        assert np.array_equal(dw.view(np.uint32), dw3.view(np.uint32)) and np.array_equal(db.view(np.uint32), db3.view(np.uint32))


def test_wgrad_centre_tap_only(ctx):
    """dilation 12 on a 9 x 9 map: the centre tap only -- the other eight are exactly 0.0 and the centre tap is x^T dz"""
    shape = (1, 9, 9, 64, 64, 3, 12)
    x, dz, (dw64, _, _, n, _) = _wgrad_case(shape)
    assert n.tolist() == [[0, 0, 0], [0, 81, 0], [0, 0, 0]]
    dw, _ = _run_wgrad(ctx, x, dz, shape, 0)
    centre = dw[1, 1].copy()
    dw[1, 1] = 0
    assert not dw.any() and np.abs(centre).max() > 0


# ---- data gradient ------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [(2, 7, 5, 64, 64, 3, 1), (1, 9, 9, 128, 64, 3, 2), (2, 9, 9, 64, 128, 3, 6), (1, 9, 9, 64, 64, 3, 12), (2, 8, 6, 128, 21, 1, 1),
               (2, 8, 6, 128, 5, 1, 1)]
# fc6, fc6_1, fc7, fc8, conv4_1 at their real widths (K = 9 x 1024 in the first two); M = 1, H = 1, W = 1; Cout = 1, padded to the
# convolution's channel granule
DGRAD_FULL_CASES = [(1, 9, 9, 512, 1024, 3, 12), (1, 9, 9, 512, 1024, 3, 6), (1, 5, 7, 1024, 1024, 1, 1), (2, 5, 7, 1024, 21, 1, 1),
                    (1, 9, 9, 256, 512, 3, 1)]
DGRAD_SMALL_CASES = [(1, 1, 1, 64, 64, 3, 1), (1, 1, 7, 64, 64, 3, 1), (2, 7, 1, 128, 64, 3, 2), (2, 5, 3, 64, 1, 1, 1)]


@pytest.mark.parametrize("case", DGRAD_CASES + DGRAD_FULL_CASES + DGRAD_SMALL_CASES, ids=_id)
def test_dgrad(ctx, case):
    N, H, W, Cin, Cout, k, dil = case
    rng = np.random.default_rng(sum(case) + 1)
    dz = (1e-3 * rng.standard_normal((N, H, W, Cout))).astype(np.float32)
    w = rng.standard_normal((k, k, Cin, Cout)).astype(np.float32)  # asymmetric in every index
    dx64, S = gref.dgrad_ref(dz, w, dil)
    with DeviceMaps.from_host(ctx, dz) as zd, _guarded(ctx, (N, H, W, Cin)) as dx:
        _lib.conv2d_dgrad_nhwc(ctx, zd.ptr, w, N, H, W, Cin, Cout, k, dil, dx.ptr)
        got = _checked(dx, (N, H, W, Cin), "dx")
    bound = (k * k * Cout + 2) * U * S
    err = np.abs(got.astype(np.float64) - dx64)
    print("dgrad %s: max err / bound %.3f, max err %.3e, max|dx| %.3e" % (_id(case), float((err / np.maximum(bound, 1e-300)).max()),
                                                                         err.max(), np.abs(dx64).max()))
    assert (err <= bound).all() and np.abs(dx64).max() > 0


# ---- ReLU mask + bias gradient -------------------------------------------------------------------------------------------------
# 70001 rows: the 1024-block cap (69 rows a block, the last blocks ragged and empty); one row; four blocks of the finish kernel; C = 2
@pytest.mark.parametrize("M, C, mask", [(70, 64, True), (3069, 192, True), (96, 21, False), (70001, 64, True), (1, 64, True), (81, 1024, True),
                                        (96, 2, False)],
                         ids=["70x64", "3069x192", "96x21-nomask", "70001x64", "1x64", "81x1024", "96x2-nomask"])
def test_relu_bias_grad(ctx, M, C, mask):
    rng = np.random.default_rng(M + C)
    y = _relu_like(rng, (M, C))
    dy = (1e-3 * rng.standard_normal((M, C))).astype(np.float32)
    dy[0, 0] = -0.0
    want = np.where(y > 0, dy, np.float32(0.0)).astype(np.float32) if mask else dy
    with DeviceMaps.from_host(ctx, y) as yd, DeviceMaps.from_host(ctx, dy) as gd, _guarded(ctx, (M, C)) as dz, _guarded(ctx, (C,)) as db:
        _lib.relu_bias_grad(ctx, yd.ptr if mask else None, gd.ptr, M, C, dz.ptr, db.ptr)
        got, gb = _checked(dz, (M, C), "dz"), _checked(db, (C,), "db")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # dy or +0.0, to the bits
    w64 = want.astype(np.float64)
    errb = np.abs(gb.astype(np.float64) - w64.sum(0))
    bound = (M + 2) * U * np.abs(w64).sum(0)
    print("relu_bias_grad %d x %d: db max err / bound %.3f" % (M, C, float((errb / np.maximum(bound, 1e-300)).max())))
    assert (errb <= bound).all()


# ---- pool gradients --------------------------------------------------------------------------------------------------------------
POOL_CASES = [(0, 2, (2, 9, 9, 64)), (0, 2, (2, 8, 6, 64)), (0, 1, (2, 9, 9, 64)), (0, 1, (1, 1, 7, 64)),
              (1, 1, (2, 9, 9, 64)), (1, 1, (2, 8, 6, 64)), (1, 1, (1, 1, 1, 64))]
# conv4 / conv5's width; W = 1; a 2 x 2 map (stride 2: one window) -- every mode
POOL_CASES += [(avg, stride, shape) for avg, stride in ((0, 2), (0, 1), (1, 1)) for shape in ((2, 5, 7, 512), (1, 7, 1, 64), (1, 2, 2, 64))]


@pytest.mark.parametrize("avg, stride, shape", POOL_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("integers", [False, True], ids=["real", "int"])
def test_pool_grad(ctx, avg, stride, shape, integers):
    N, H, W, C = shape
    rng = np.random.default_rng(sum(shape) + 10 * stride + avg)
    x = _relu_like(rng, shape)
    Ho, Wo = gref.pool_out_hw(H, W, stride)
    dy = rng.integers(-3, 4, (N, Ho, Wo, C)).astype(np.float32) if integers else (1e-3 * rng.standard_normal((N, Ho, Wo, C))).astype(np.float32)
    dx64, S = gref.pool_grad_ref(x, dy, avg, stride)
    with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, dy) as gd, _guarded(ctx, shape) as dx:
        _lib.pool_same_grad_nhwc(ctx, xd.ptr, gd.ptr, N, H, W, C, avg, stride, dx.ptr)
        got = _checked(dx, shape, "pool dx")
    err = np.abs(got.astype(np.float64) - dx64)
    bound = (9 + 2) * U * S
    print("pool grad avg=%d stride=%d %s: max err %.3e, max err / bound %.3f" % (avg, stride, _id(shape), err.max(),
                                                                                float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    if integers and not avg:
        assert np.array_equal(got.astype(np.float64), dx64)  # sums of small integers: exact


# ---- the tape --------------------------------------------------------------------------------------------------------------------
def _check_tape(ctx, method, prec, weights, x, C):
    B, hw = x.shape[0], x.shape[1:3]
    net = secdsrg.SegNet(method, weights, C, precision=prec, ctx=ctx)
    try:
        with DeviceMaps.from_host(ctx, x) as xd:
            p0, f0 = net.forward_dev(xd, want_fc8=True)
            p1, f1, tape = net.forward_dev(xd, want_fc8=True, keep=True)
            with p0, f0, p1, f1, tape:
                assert np.array_equal(p0.to_host().view(np.uint32), p1.to_host().view(np.uint32))
                assert np.array_equal(f0.to_host().view(np.uint32), f1.to_host().view(np.uint32))
                flat = tape.to_host()
                ops = net.net.trace_plan(B, hw[0], hw[1])
                offs, n = [], 0
                for o in ops:
                    offs.append(n)
                    n += B * o["Ho"] * o["Wo"] * o["pitch"]
                with DeviceMaps(ctx, (n,), np.float32) as tr:
                    net.net.forward_trace(xd.ptr, B, hw[0], hw[1], offs, tr.ptr, n)
                    trace = tr.to_host()
                entries = tape.entries
                assert [e["name"] for e in entries[:1 + len(ops)]] == ["input"] + [o["label"] for o in ops[:-1]] + ["pool5a"]
                assert [e["name"] for e in entries[1 + len(ops):]] == [l for l in ref.layer_names(method) if l[:3] in ("fc6", "fc7")]
                for e, o, off in zip(entries[1:], ops, offs):
                    cnt = B * o["Ho"] * o["Wo"] * o["pitch"]
                    assert (e["Ho"], e["Wo"], e["C"]) == (o["Ho"], o["Wo"], o["pitch"])
                    assert np.array_equal(flat[e["offset"]:e["offset"] + cnt].view(np.uint32), trace[off:off + cnt].view(np.uint32)), e["name"]
                e0 = entries[0]
                got_in = flat[e0["offset"]:e0["offset"] + x.size].reshape(x.shape)
                if prec == _lib.PREC_F32:
                    assert np.array_equal(got_in, x)
                else:  # hi + lo of two halves: 22 bits of the input
                    assert np.abs(got_in - x).max() <= 2.0 ** -21 * np.abs(x).max()
    finally:
        net.close()


@pytest.mark.parametrize("prec", [_lib.PREC_F16X3, _lib.PREC_F32], ids=["f16x3", "f32"])
@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_tape_is_the_forward_pass(ctx, method, prec):
    """forward_seg_tape's fc8 / prob have wsc_net_forward_seg's bits, its trunk entries wsc_net_forward_trace's"""
    C, hw = 5, (64, 48)
    weights, x = ref.thin_case(method, C, hw)
    _check_tape(ctx, method, prec, weights, x, C)


def test_tape_is_the_forward_pass_full_width(ctx):
    """the same at the real widths: DSRG, 21 classes, 65 x 65, B = 1, f16x3"""
    weights, x = gref.full_case(("DSRG", 21, (65, 65), 1))
    _check_tape(ctx, "DSRG", _lib.PREC_F16X3, weights, x, 21)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _tape_dict(tape, flat):
    B = tape.input_shape[0]
    return {e["name"]: flat[e["offset"]:e["offset"] + B * e["Ho"] * e["Wo"] * e["C"]].reshape(B, e["Ho"], e["Wo"], e["C"]) for e in tape.entries}


def _case_id(case):
    return "%s-%d-%dx%d" % (case[0], case[1], case[2][0], case[2][1])


@pytest.mark.parametrize("prec", [_lib.PREC_F32, _lib.PREC_F16X3], ids=["f32", "f16x3"])
@pytest.mark.parametrize("case", gref.GRAD_CASES, ids=_case_id)
def test_backward_seg_end_to_end(ctx, case, prec):
    method, C, hw = case
    weights, x = ref.thin_case(method, C, hw)
    net = secdsrg.SegNet(method, weights, C, precision=prec, ctx=ctx)
    try:
        prob, tape = net.forward_dev(x, keep=True)
        with prob, tape:
            rng = np.random.default_rng(900 + 3 * C + hw[1] + (1 if method == "SEC" else 0))
            dfc8 = (1e-3 * rng.standard_normal(prob.shape)).astype(np.float32)
            with net.backward_dev(tape, dfc8) as grads:
                got = grads.to_host()
                with net.backward_dev(tape, dfc8) as again:  # two calls: the same bits
                    assert np.array_equal(grads.maps.to_host().view(np.uint32), again.maps.to_host().view(np.uint32))
            want = gref.chain_grads(method, weights, _tape_dict(tape, tape.to_host()), dfc8, torch.float64)
    finally:
        net.close()
    assert set(got) == set(ref.layer_names(method))
    ratios = gref.layer_ratio(got, want)
    layer = max(ratios, key=lambda l: max(ratios[l]))
    print("backward_seg %s %s: worst max|d| / max|g64| = %.3e at %s (bound %.3e = 64 R32_CHAIN)"
          % (_case_id(case), "f32" if prec == _lib.PREC_F32 else "f16x3", max(ratios[layer]), layer, 64 * gref.R32_CHAIN))
    for name, (rw, rb) in ratios.items():
        assert got[name]["w"].shape == np.shape(weights[name]["w"]) and got[name]["b"].shape == (np.shape(weights[name]["w"])[3],)
        assert rw <= 64 * gref.R32_CHAIN and rb <= 64 * gref.R32_CHAIN, (name, rw, rb)
    if method == "SEC" and hw in ((65, 65), (97, 97)):
        w6 = got["fc6"]["w"]
        live = [[bool(w6[r, s].any()) for s in range(3)] for r in range(3)]
        if hw == (65, 65):  # a 9 x 9 map at rate 12: the centre tap only, the others exactly zero
            assert live == [[False, False, False], [False, True, False], [False, False, False]]
        else:               # 13 x 13: all nine
            assert all(all(row) for row in live)


def _full_id(case):
    return "%s-%d-%dx%d-B%d" % (case[0], case[1], case[2][0], case[2][1], case[3])


CENTRE_TAP = [[False, False, False], [False, True, False], [False, False, False]]
MIDDLE_COLUMN = [[False, True, False], [False, True, False], [False, True, False]]
ALL_TAPS = [[True, True, True], [True, True, True], [True, True, True]]


def _layer_grads(flat, layout):
    """the gradient buffer on the host -> {layer: {'w': HWIO view, 'b': view}}"""
    out = {}
    for layer, e in layout.items():
        nw = e["k"] * e["k"] * e["Cin"] * e["Cout"]
        out[layer] = {"w": flat[e["w_off"]:e["w_off"] + nw].reshape(e["k"], e["k"], e["Cin"], e["Cout"]),
                      "b": flat[e["b_off"]:e["b_off"] + e["Cout"]]}
    return out


@pytest.mark.parametrize("prec", [_lib.PREC_F32, _lib.PREC_F16X3], ids=["f32", "f16x3"])
@pytest.mark.parametrize("case", gref.FULL_GRAD_CASES, ids=_full_id)
def test_backward_seg_end_to_end_full_width(ctx, case, prec):
    """test_backward_seg_end_to_end at the real widths (64 ... 512, fc 1024, 21 classes): the tile counts, the fc8 form, K = 9 x 1024
    in the data gradient, the finish kernel on several blocks and a workspace whose parts are sized by different layers.  The
    gradient buffer has a guard band behind it.  Per layer max|d| <= 64 R32_CHAIN_FULL max|g64|, the constant from the CPU oracle."""
    method, C, hw, B = case
    weights, x = gref.full_case(case)
    net = secdsrg.SegNet(method, weights, C, precision=prec, ctx=ctx)
    sg = None
    try:
        prob, tape = net.forward_dev(x, keep=True)
        with prob, tape:
            assert prob.shape[0] == B
            dfc8 = gref.full_dfc8(case, prob.shape)
            sg = _lib.SegGrad(net.net, net._sd)
            with DeviceMaps.from_host(ctx, dfc8) as gd:
                flats = []
                for _ in range(2):
                    with _guarded(ctx, (sg.grad_elems,)) as grad:
                        sg.backward(B, hw[0], hw[1], tape.ptr, tape.shape[0], gd.ptr, grad.ptr, grad_elems=sg.grad_elems)
                        flats.append(_checked(grad, (sg.grad_elems,), "the gradient buffer"))
            assert np.array_equal(flats[0].view(np.uint32), flats[1].view(np.uint32))  # two calls: the same bits
            got = _layer_grads(flats[0], sg.layout)
            del flats
            want = gref.chain_grads(method, weights, _tape_dict(tape, tape.to_host()), dfc8, torch.float64)
    finally:
        if sg is not None:
            sg.close()
        net.close()
    assert set(got) == set(ref.layer_names(method))
    ratios = gref.layer_ratio(got, want)
    layer = max(ratios, key=lambda l: max(ratios[l]))
    smallest = min(min(np.abs(g["w"]).max(), np.abs(g["b"]).max()) for g in want.values())
    print("backward_seg full width %s %s: worst max|d| / max|g64| = %.3e at %s (bound %.3e = 64 R32_CHAIN_FULL); smallest max|g64| %.3e"
          % (_full_id(case), "f32" if prec == _lib.PREC_F32 else "f16x3", max(ratios[layer]), layer, 64 * gref.R32_CHAIN_FULL, smallest))
    assert smallest > 0  # every layer has a gradient to be compared with
    for name, (rw, rb) in ratios.items():
        assert got[name]["w"].shape == np.shape(weights[name]["w"]) and got[name]["b"].shape == (np.shape(weights[name]["w"])[3],)
        assert rw <= 64 * gref.R32_CHAIN_FULL and rb <= 64 * gref.R32_CHAIN_FULL, (name, rw, rb)
    for sfx, _ in gref.branches(method):  # fc6's live taps: what the map size leaves in the image; a dead tap is +0.0 everywhere
        w6 = got["fc6" + sfx]["w"]
        live = [[bool(w6[r, s].any()) for s in range(3)] for r in range(3)]
        assert live == (CENTRE_TAP if sfx != "_1" else ALL_TAPS if hw == (65, 65) else MIDDLE_COLUMN), ("fc6" + sfx, live)
        assert not any(np.signbit(w6[r, s]).any() for r in range(3) for s in range(3) if not live[r][s])


# ---- batch sizes, one workspace at several sizes ----------------------------------------------------------------------------------
THIN = ("DSRG", 5, (65, 65))


def _backward_host(net, x, seed):
    """forward_dev(keep) + backward_dev of a SegNet on x with dfc8 = 1e-3 N(0, 1) of `seed` -> (flat gradient, the tape as a dict, dfc8)"""
    prob, tape = net.forward_dev(x, keep=True)
    with prob, tape:
        dfc8 = (1e-3 * np.random.default_rng(seed).standard_normal(prob.shape)).astype(np.float32)
        with net.backward_dev(tape, dfc8) as grads:
            return grads.maps.to_host(), _tape_dict(tape, tape.to_host()), dfc8


@pytest.mark.parametrize("B", [1, 3])
def test_backward_seg_batch_sizes(ctx, B):
    """the thin DSRG net at B = 1 (the first image of thin_case's input) and B = 3: test_backward_seg_end_to_end's bound, f32"""
    method, C, hw = THIN
    weights, x2 = ref.thin_case(method, C, hw)
    x = x2[:1] if B == 1 else ref.net_input(3, hw[0], hw[1], 100 + 7 * C + hw[1] + 1)
    net = secdsrg.SegNet(method, weights, C, precision=_lib.PREC_F32, ctx=ctx)
    try:
        flat, tape, dfc8 = _backward_host(net, x, 950 + B)
        got = _layer_grads(flat, net._grad.layout)
    finally:
        net.close()
    assert dfc8.shape == (B, 9, 9, C)
    want = gref.chain_grads(method, weights, tape, dfc8, torch.float64)
    ratios = gref.layer_ratio(got, want)
    layer = max(ratios, key=lambda l: max(ratios[l]))
    print("backward_seg thin DSRG 65x65 B=%d f32: worst max|d| / max|g64| = %.3e at %s (bound %.3e = 64 R32_CHAIN)"
          % (B, max(ratios[layer]), layer, 64 * gref.R32_CHAIN))
    assert set(got) == set(ref.layer_names(method))
    for name, (rw, rb) in ratios.items():
        assert np.abs(want[name]["w"]).max() > 0 and np.abs(want[name]["b"]).max() > 0
        assert rw <= 64 * gref.R32_CHAIN and rb <= 64 * gref.R32_CHAIN, (name, rw, rb)


def _tracked_grad_step(ctx, monkeypatch, net, x, cues, tags):
    """grad_step_dev with every allocation of the context recorded -> (losses, grads, new_cues, the buffers still live after it)"""
    handed = []
    alloc0 = ctx.alloc

    def alloc(nbytes, pooled=False):
        handed.append(alloc0(nbytes, pooled=pooled))
        return handed[-1]

    monkeypatch.setattr(ctx, "alloc", alloc)
    losses, grads, new_cues = net.grad_step_dev(x, cues, tags, MEAN, CRF_CFG)
    monkeypatch.undo()
    return losses, grads, new_cues, [b for b in handed if b.ptr is not None]


def test_backward_seg_workspace_reuse(ctx, monkeypatch):
    """One SegNet (thin DSRG, f32) at 64 x 48, 97 x 97 (the workspace grows: sync, free, malloc, re-carve) and 64 x 48 again: every
    result has the bits a fresh SegNet gives at that size, and grad_step_dev afterwards hands every buffer back."""
    method, C, _ = THIN
    weights, x65 = ref.thin_case(method, C, (65, 65))
    sizes = [(64, 48), (97, 97), (64, 48)]
    xs = {hw: ref.net_input(2, hw[0], hw[1], 300 + hw[1]) for hw in set(sizes)}
    net = secdsrg.SegNet(method, weights, C, precision=_lib.PREC_F32, ctx=ctx)
    try:
        got = [_backward_host(net, xs[hw], 400 + hw[1])[0] for hw in sizes]
        assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))
        assert not np.array_equal(got[0], got[1]) and np.abs(got[1]).max() > 0
        for hw, g in zip(sizes[:2], got[:2]):
            fresh = secdsrg.SegNet(method, weights, C, precision=_lib.PREC_F32, ctx=ctx)
            try:
                assert np.array_equal(_backward_host(fresh, xs[hw], 400 + hw[1])[0].view(np.uint32), g.view(np.uint32)), hw
            finally:
                fresh.close()
        rng = np.random.default_rng(78)
        cues = (rng.random((2, 9, 9, C)) < 0.2).astype(np.float32)
        tags = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 1]], np.float32)
        losses, grads, new_cues, live = _tracked_grad_step(ctx, monkeypatch, net, x65, cues, tags)
        with grads, new_cues:
            assert sorted(b.ptr for b in live) == sorted([grads.maps.ptr, new_cues.ptr])
            assert np.abs(grads.maps.to_host()).max() > 0
    finally:
        net.close()


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_grad_step_dev(ctx, monkeypatch):
    """grad_step_dev: loss_step_dev's losses bit for bit, the gradients backward_dev gives for its tape and gradient, and every
    buffer of the step handed back"""
    method, C = "DSRG", 5
    weights, x = ref.thin_case(method, C, (65, 65))
    rng = np.random.default_rng(77)
    cues = (rng.random((2, 9, 9, C)) < 0.2).astype(np.float32)
    tags = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 1]], np.float32)
    net = secdsrg.SegNet(method, weights, C, ctx=ctx)
    try:
        want_l, want_g, want_c = net.loss_step_dev(x, cues, tags, MEAN, CRF_CFG)
        prob, tape = net.forward_dev(x, keep=True)
        with want_g, want_c, prob, tape, net.backward_dev(tape, want_g) as want:
            losses, grads, new_cues, live = _tracked_grad_step(ctx, monkeypatch, net, x, cues, tags)
            assert sorted(b.ptr for b in live) == sorted([grads.maps.ptr, new_cues.ptr])  # the tape, d loss / d fc8, ... went back
            with grads, new_cues:
                assert losses == want_l  # to the bits
                assert np.array_equal(new_cues.to_host(), want_c.to_host())
                assert np.array_equal(grads.maps.to_host().view(np.uint32), want.maps.to_host().view(np.uint32))
                one = grads["fc7_3"]
                assert one["w"].shape == (1, 1, 128, 128) and one["b"].shape == (128,)
                assert np.array_equal(one["w"], grads.to_host()["fc7_3"]["w"]) and np.abs(one["w"]).max() > 0
                assert grads.ptr("fc7_3", "b") == grads.maps.ptr + 4 * grads.layout["fc7_3"]["b_off"]
        assert net._grad is not None
    finally:
        net.close()
    assert net._grad is None


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(ctx):
    C = 5
    weights, x = ref.thin_case("DSRG", C, (65, 65))
    net = secdsrg.SegNet("DSRG", weights, C, precision=_lib.PREC_F32, ctx=ctx)
    try:
        entries, elems = net.net.seg_tape_plan(2, 65, 65)
        sg = _lib.SegGrad(net.net, net._sd)
        canary = np.full((sg.grad_elems,), CANARY, np.float32)
        with DeviceMaps(ctx, (elems,), np.float32) as tape, DeviceMaps.from_host(ctx, np.zeros((2, 9, 9, C), np.float32)) as g8, \
                DeviceMaps.from_host(ctx, canary) as grad, DeviceMaps.from_host(ctx, x) as xd, DeviceMaps(ctx, (2, 9, 9, C), np.float32) as prob:
            for kw in ({"tape_elems": elems - 64}, {"grad_elems": sg.grad_elems - 1}):
                with pytest.raises(_lib.WscError) as ei:
                    sg.backward(2, 65, 65, tape.ptr, kw.get("tape_elems", elems), g8.ptr, grad.ptr, grad_elems=kw.get("grad_elems"))
                assert ei.value.status == _lib.WSC_ERR_INVALID
            with pytest.raises(_lib.WscError) as ei:  # a short tape in the forward pass
                net.net.forward_seg_tape(xd.ptr, 2, 65, 65, tape.ptr, elems - 64, prob.ptr)
            assert ei.value.status == _lib.WSC_ERR_INVALID
            other = _lib.Context(0)  # the workspace belongs to the stream of the context the object was created on
            try:
                with pytest.raises(_lib.WscError) as ei:
                    _lib.check(ctx._lib.wsc_net_backward_seg(other.h, sg.h, 2, 65, 65, tape.ptr, elems, g8.ptr, grad.ptr, sg.grad_elems))
                assert ei.value.status == _lib.WSC_ERR_INVALID
            finally:
                other.close()
            assert np.array_equal(grad.to_host(), canary)  # nothing was launched
        sg.close()
        bad = dict(net._sd)
        bad["fc7_3.w"] = np.zeros((1, 1, 128, 64), np.float32)
        with pytest.raises(_lib.WscError) as ei:
            _lib.SegGrad(net.net, bad)
        assert ei.value.status == _lib.WSC_ERR_SHAPE and "fc7_3" in str(ei.value)
    finally:
        net.close()
    # a CAM net has no tape and no backward pass
    sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
    cam = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, sd, 20, _lib.PREC_F16)
    try:
        with pytest.raises(_lib.WscError) as ei:
            cam.seg_tape_plan(1, 65, 65)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        with pytest.raises(_lib.WscError) as ei:
            _lib.SegGrad(cam, sd)
        assert ei.value.status == _lib.WSC_ERR_INVALID
    finally:
        cam.close()
