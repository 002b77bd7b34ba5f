"""GPU: the training pass of the plain stacks (VGG16 / M7) -- BatchNorm in training mode (csrc/cls_grad.hip), the pool gradients of
the Keras / torch pool family (csrc/pool.hip), wsc_net_forward_cls_train / wsc_net_backward_cls (csrc/net.hip), and
vgg16_cam.CAM.forward_train_dev / backward_dev, cls_train.grad_step -- against the float64 oracle tests/cls_grad_ref.py.

u = 2^-24, v = 2^-53 throughout.  The per-op tests compare with float64 on the identical float32 operands, elementwise, with bounds
from the arithmetic the header states; each holds for any summation order.  With d = a - a[0] (the kernel's pivot), r = rstd,
g = gamma:
  mean      u |mean| + (M + 2) v (|a[0]| + sum|d| / M): one float rounding of a double sum of M terms
  rstd      r (u + dvar / (2 (var + eps))), dvar = 2 (M + 2) v (sum d^2 / M + (sum|d| / M)^2): the double sums, then one float rounding
  y         (3 + 2) u (|g| r |mean| + |g| r |a - mean| + |y|) + |g| r |a - mean| dvar / (2 (var + eps)): the float rounding of the
            mean as the difference sees it, the roundings of the difference, of rstd and of the product, the fma's one rounding
  running   u |want| + (1 - keep) (the mean's / dvar M / (M - 1)) double error: formed in double from the unrounded batch values
  dbeta     u |dbeta| + (M + 2) v sum|dy|
  dgamma    (2 + 2) u sum|dy xh|: xh carries the roundings of its difference and its product
  da        |g r| ((6 + 2) u (|dy| + |mb| + |xh mg|) + |xh| (2 + 2) u sum|dy xh| / M): at most six roundings on a term (xh's two, mg's,
            the fma's, g r's, the product's), and mg inherits dgamma's absolute error
  a constant channel is exact: mean = the value, rstd = float(1 / sqrt(eps)), y = beta, dgamma = 0
  pool gradients  dy of small integers: the float64 result exactly
The whole pass at WSC_PREC_F32 and at f16x3: every gradient tensor within 64 R32_CHAIN_CLS max|g64| of chain_grads(float64) on the
device's own downloaded tape (the project's margin for an end-to-end backward: it guards the wiring, the arithmetic is held by the
per-op bounds); the tape itself against the float64 op on the entries it read: convolutions at net_trace_ref.asserted_bound (the
suite's per-precision bound of tests/test_gpu_net_trace.py), pools equal, BatchNorm at the bound above plus the planes' split
(2^-22 |y| + 2^-25 in f16x3), statistics within 2^-23 relative.  Every test prints the figure it asserts on.

Every device output of a per-op test has GUARD floats of CANARY behind it that must survive, and must be overwritten entirely."""
import functools

import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import cls_grad_ref as gref
from tests import net_trace_ref as nt
from wsscam import _lib, cls_train
from wsscam.net import m7_cam, vgg16_cam
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

U, V = 2.0 ** -24, 2.0 ** -53
CANARY = np.float32(-777.25)
GUARD = 256  # floats of CANARY behind every device output
EPS32 = float(np.float32(gref.EPS))  # the eps the kernels see
KEEP32 = float(np.float32(0.99))
PRECS = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3}


def _canary(ctx, shape):
    return DeviceMaps.from_host(ctx, np.full((int(np.prod(shape)) + GUARD,), CANARY, np.float32))


def _guarded(ctx, a):
    """a host array on the device with GUARD canaries behind it"""
    return DeviceMaps.from_host(ctx, np.concatenate([np.ascontiguousarray(a, np.float32).ravel(), np.full((GUARD,), CANARY, np.float32)]))


def _checked(buf, shape, what, written=True):
    flat = buf.to_host().ravel()
    n = int(np.prod(shape))
    assert flat.size == n + GUARD
    assert np.array_equal(flat[n:].view(np.uint32), np.full((GUARD,), CANARY, np.float32).view(np.uint32)), what + ": a store behind the output"
    if written:
        assert not (flat[:n] == CANARY).any(), what + ": an element was not written"
    return flat[:n].reshape(shape).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- BatchNorm, forward and backward ---------------------------------------------------------------------------------------------
# (M, C): B = 2 at 1 x 1; 2 x 3 x 5; 3 x 9 x 11 = 297 rows -- five blocks of 60 rows, the last one of 57; a slab of 8 channels
# behind a full one (C = 72); the widest layer
BN_CASES = [(2, 64), (30, 64), (297, 64), (30, 72), (2, 1024), (30, 1024), (297, 1024)]


@functools.lru_cache(maxsize=None)
def bn_case(M, C):
    """(a, gamma, beta, dy, run0): channel 0 constant, channel 1 of mean 1e3 and std 1e-2, some negative gammas; shared, never modified"""
    rng = np.random.default_rng(31 * M + C)
    a = (2.0 * rng.standard_normal((M, C)) + 0.5).astype(np.float32)
    a[:, 0] = 3.25
    a[:, 1] = (1e3 + 1e-2 * rng.standard_normal(M)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.2, -1.0, 1.0)).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    dy = rng.standard_normal((M, C)).astype(np.float32)
    run0 = np.stack([rng.standard_normal(C), rng.uniform(0.5, 2.0, C)]).astype(np.float32)
    return a, gamma, beta, dy, run0


def run_bn_train(ctx, a, gamma, beta, run0, keep=0.99, unbiased=True):
    """-> (stats (C, 2), y (M, C), run (2, C) or None)"""
    M, C = a.shape
    with _guarded(ctx, a) as ad, DeviceMaps.from_host(ctx, gamma) as gd, DeviceMaps.from_host(ctx, beta) as bd, _canary(ctx, (C, 2)) as st, \
            _canary(ctx, (M, C)) as y:
        if run0 is None:
            _lib.batch_norm_train_nhwc(ctx, ad.ptr, M, C, gd.ptr, bd.ptr, gref.EPS, keep, unbiased, None, st.ptr, y.ptr)
            return _checked(st, (C, 2), "stats"), _checked(y, (M, C), "y"), None
        with _guarded(ctx, run0) as run:
            _lib.batch_norm_train_nhwc(ctx, ad.ptr, M, C, gd.ptr, bd.ptr, gref.EPS, keep, unbiased, run.ptr, st.ptr, y.ptr)
            return _checked(st, (C, 2), "stats"), _checked(y, (M, C), "y"), _checked(run, (2, C), "run")


def run_bn_grad(ctx, a, stats, gamma, dy):
    M, C = a.shape
    with _guarded(ctx, a) as ad, _guarded(ctx, dy) as dd, DeviceMaps.from_host(ctx, stats) as st, DeviceMaps.from_host(ctx, gamma) as gd, \
            _canary(ctx, (M, C)) as da, _canary(ctx, (C,)) as dg, _canary(ctx, (C,)) as db:
        _lib.batch_norm_grad_nhwc(ctx, ad.ptr, st.ptr, gd.ptr, dd.ptr, M, C, da.ptr, dg.ptr, db.ptr)
        return _checked(da, (M, C), "da"), _checked(dg, (C,), "dgamma"), _checked(db, (C,), "dbeta")


def bn_bounds(a, gamma, mean, var, rstd, y):
    """(the bounds of mean, rstd, y; the double errors of mean and var) -- the docstring's formulas, float64 arrays"""
    M = a.shape[0]
    a64, g = a.astype(np.float64), np.abs(gamma.astype(np.float64))
    d = np.abs(a64 - a64[0])
    dmean = (M + 2) * V * (np.abs(a64[0]) + d.sum(0) / M)
    dvar = 2 * (M + 2) * V * ((d * d).sum(0) / M + (d.sum(0) / M) ** 2)
    rel = dvar / (2 * (var + EPS32))
    t1, t2, t3 = g * rstd * np.abs(mean), g * rstd * np.abs(a64 - mean), np.abs(y)
    return U * np.abs(mean) + dmean, rstd * (U + rel) * (1 + 1e-6), 5 * U * (t1 + t2 + t3) + t2 * rel, dmean, dvar


@pytest.mark.parametrize("with_run", [False, True], ids=["norun", "run"])
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%dx%d" % c)
def test_batch_norm_train(ctx, case, with_run):
    M, C = case
    a, gamma, beta, _, run0 = bn_case(M, C)
    mean, var, rstd, y64 = gref.bn_train_ref(a, gamma, beta, EPS32)
    b_mean, b_rstd, b_y, dmean, dvar = bn_bounds(a, gamma, mean, var, rstd, y64)
    stats, y, run = run_bn_train(ctx, a, gamma, beta, run0 if with_run else None)
    e_mean, e_rstd, e_y = np.abs(stats[:, 0] - mean), np.abs(stats[:, 1] - rstd), np.abs(y.astype(np.float64) - y64)
    print("batch_norm_train %dx%d: max err / bound mean %.3f rstd %.3f y %.3f (cancellation channel: rstd err %.2e of %.3f, y err / bound %.3f)" % (
        M, C, (e_mean / b_mean).max(), (e_rstd / b_rstd).max(), (e_y / np.maximum(b_y, 1e-300)).max(), e_rstd[1], rstd[1],
        (e_y[:, 1] / b_y[:, 1]).max()))
    assert (e_mean <= b_mean).all() and (e_rstd <= b_rstd).all() and (e_y <= b_y).all()
    # the constant channel is exact
    assert stats[0, 0] == np.float32(3.25) and stats[0, 1] == np.float32(1.0 / np.sqrt(EPS32)) and np.array_equal(_bits(y[:, 0]), _bits(np.full(M, beta[0])))
    # y is the header's expression on the float statistics, to the bit
    xh = ((a - stats[:, 0]) * stats[:, 1]).astype(np.float32)
    want = (xh.astype(np.longdouble) * gamma.astype(np.longdouble) + beta.astype(np.longdouble)).astype(np.float32)  # (the fma's one rounding)
    assert np.array_equal(_bits(y), _bits(want))
    again = run_bn_train(ctx, a, gamma, beta, run0 if with_run else None)
    assert np.array_equal(_bits(stats), _bits(again[0])) and np.array_equal(_bits(y), _bits(again[1]))
    if not with_run:
        return
    assert np.array_equal(_bits(run), _bits(again[2]))
    plain = run_bn_train(ctx, a, gamma, beta, None)  # the running statistics change nothing else
    assert np.array_equal(_bits(stats), _bits(plain[0])) and np.array_equal(_bits(y), _bits(plain[1]))
    r0 = run0.astype(np.float64)
    want_run = np.stack([KEEP32 * r0[0] + (1 - KEEP32) * mean, KEEP32 * r0[1] + (1 - KEEP32) * var * M / (M - 1)])
    b_run = U * np.abs(want_run) + (1 - KEEP32) * np.stack([dmean, dvar * M / (M - 1)]) + 4 * V * (np.abs(r0) + np.abs(want_run))
    e_run = np.abs(run.astype(np.float64) - want_run)
    print("       running statistics: max err / bound %.3f" % (e_run / b_run).max())
    assert (e_run <= b_run).all()
    biased = run_bn_train(ctx, a, gamma, beta, run0, keep=0.25, unbiased=False)[2].astype(np.float64)
    want_b = 0.25 * r0[1] + 0.75 * var
    assert (np.abs(biased[1] - want_b) <= U * np.abs(want_b) + 0.75 * dvar + 4 * V * (np.abs(r0[1]) + want_b)).all()


@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%dx%d" % c)
def test_batch_norm_grad(ctx, case):
    M, C = case
    a, gamma, beta, dy, _ = bn_case(M, C)
    mean, var, rstd, _ = gref.bn_train_ref(a, gamma, beta, EPS32)
    stats = np.stack([mean, rstd], 1).astype(np.float32)  # the taped floats
    da64, dg64, db64, xh = gref.bn_grad_ref(a, stats, gamma, dy)
    da, dg, db = run_bn_grad(ctx, a, stats, gamma, dy)
    dy64, g, r = dy.astype(np.float64), np.abs(gamma.astype(np.float64)), stats[:, 1].astype(np.float64)
    S = np.abs(dy64 * xh).sum(0)
    b_db = U * np.abs(db64) + (M + 2) * V * np.abs(dy64).sum(0)
    b_dg = 4 * U * S
    b_da = g * r * (8 * U * (np.abs(dy64) + np.abs(db64) / M + np.abs(xh * dg64) / M) + np.abs(xh) * 4 * U * S / M)
    e_db, e_dg, e_da = np.abs(db - db64), np.abs(dg - dg64), np.abs(da.astype(np.float64) - da64)
    print("batch_norm_grad %dx%d: max err / bound dbeta %.3f dgamma %.3f da %.3f" % (
        M, C, (e_db / b_db).max(), (e_dg[1:] / b_dg[1:]).max(), (e_da / b_da).max()))
    assert (e_db <= b_db).all() and (e_dg <= b_dg).all() and (e_da <= b_da).all()
    assert dg[0] == 0.0 and np.abs(da64).max() > 0  # the constant channel: xh = 0 exactly
    again = run_bn_grad(ctx, a, stats, gamma, dy)
    for x, y in zip((da, dg, db), again):
        assert np.array_equal(_bits(x), _bits(y))


def test_batch_norm_refusals(ctx):
    """every refusal is WSC_ERR_INVALID with nothing written"""
    a, gamma, beta, dy, run0 = bn_case(30, 64)
    with DeviceMaps.from_host(ctx, a) as ad, DeviceMaps.from_host(ctx, gamma) as gd, DeviceMaps.from_host(ctx, beta) as bd, \
            _canary(ctx, (64, 2)) as st, _canary(ctx, (30, 64)) as y, _guarded(ctx, run0) as run:
        calls = [lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 1, 64, gd.ptr, bd.ptr, gref.EPS, 0.99, True, run.ptr, st.ptr, y.ptr),  # M = 1, unbiased
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 1, 64, gd.ptr, bd.ptr, gref.EPS, 0.99, True, None, st.ptr, y.ptr),
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 30, 62, gd.ptr, bd.ptr, gref.EPS, 0.99, True, None, st.ptr, y.ptr),  # C % 4
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 1, 1028, gd.ptr, bd.ptr, gref.EPS, 0.99, False, None, st.ptr, y.ptr),  # C > 1024
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 30, 64, gd.ptr, bd.ptr, gref.EPS, 1.5, True, run.ptr, st.ptr, y.ptr),  # keep
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 30, 64, gd.ptr, bd.ptr, -1.0, 0.99, True, None, st.ptr, y.ptr),  # eps
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr, 30, 64, None, bd.ptr, gref.EPS, 0.99, True, None, st.ptr, y.ptr),
                 lambda: _lib.batch_norm_train_nhwc(ctx, ad.ptr + 4, 29, 64, gd.ptr, bd.ptr, gref.EPS, 0.99, True, None, st.ptr, y.ptr),  # alignment
                 lambda: _lib.batch_norm_grad_nhwc(ctx, ad.ptr, st.ptr, gd.ptr, ad.ptr, 30, 62, y.ptr, st.ptr, st.ptr),
                 lambda: _lib.batch_norm_grad_nhwc(ctx, ad.ptr, st.ptr, gd.ptr, None, 30, 64, y.ptr, st.ptr, st.ptr)]
        for call in calls:
            with pytest.raises(_lib.WscError) as ei:
                call()
            assert ei.value.status == _lib.WSC_ERR_INVALID
        ctx.sync()
        assert (st.to_host() == CANARY).all() and (y.to_host() == CANARY).all()
        assert np.array_equal(_bits(_checked(run, (2, 64), "run", written=False)), _bits(run0))
        # M = 1 is served where nothing asks for the unbiased variance: var = 0, y = beta
        _lib.batch_norm_train_nhwc(ctx, ad.ptr, 1, 64, gd.ptr, bd.ptr, gref.EPS, 0.99, False, run.ptr, st.ptr, y.ptr)
        stats = _checked(st, (64, 2), "stats")
        assert np.array_equal(_bits(stats[:, 0]), _bits(a[0])) and (stats[:, 1] == np.float32(1.0 / np.sqrt(EPS32))).all()
        assert np.array_equal(_bits(y.to_host()[:64]), _bits(beta))


# ---- pool gradients ----------------------------------------------------------------------------------------------------------------
# every (window, stride, padding) a `pool_spec` row may hold, and torch's MaxPool2d(2, 2)
POOLS = [("tf", k, s, same) for k in (2, 3) for s in (1, 2) for same in (0, 1)] + [("torch", 2, 2, 0)]
POOL_MAPS = [(7, 9), (8, 6)]


@functools.lru_cache(maxsize=None)
def pool_case(pool, hw, fill):
    """(x, dy, the float64 dx): x post-ReLU-like (half zeros, repeated maxima among the multiples of 1 / 4) or all zeros, dy small
    integers, so that the result is exact"""
    rng = np.random.default_rng(hash((pool[1:], hw)) % 1000 + len(fill))
    N, C = 2, 16
    x = (np.maximum(rng.integers(-8, 9, (N,) + hw + (C,)), 0) / 4.0).astype(np.float32) if fill == "relu" else np.zeros((N,) + hw + (C,), np.float32)
    dy = rng.integers(-4, 5, (N,) + gref.pool_out_hw(hw[0], hw[1], pool) + (C,)).astype(np.float32)
    return x, dy, gref.pool_grad_ref(x, dy, pool)


def run_pool_grad(ctx, x, dy, pool):
    N, H, W, C = x.shape
    kind, k, stride, last = pool
    with _guarded(ctx, x) as xd, _guarded(ctx, dy) as dd, _canary(ctx, x.shape) as dx:
        (_lib.pool_tf_grad_nhwc if kind == "tf" else _lib.maxpool_grad_nhwc)(ctx, xd.ptr, dd.ptr, N, H, W, C, k, stride, last, dx.ptr)
        return _checked(dx, x.shape, "dx")


@pytest.mark.parametrize("fill", ["relu", "zero"])
@pytest.mark.parametrize("hw", POOL_MAPS, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("pool", POOLS, ids=lambda p: "%s-%d-%d-%d" % p)
def test_pool_grad(ctx, pool, hw, fill):
    x, dy, want = pool_case(pool, hw, fill)
    got = run_pool_grad(ctx, x, dy, pool)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(_bits(got), _bits(run_pool_grad(ctx, x, dy, pool)))
    assert got.sum() == dy.sum() and np.abs(dy).max() > 0  # every window's dy lands on exactly one tap
    if pool[1:] == (2, 2, 0) and hw == (7, 9):  # VALID / torch 2 x 2 / 2 on 7 x 9: the last row and column belong to no window
        assert not got[:, 6].any() and not got[:, :, 8].any() and not np.signbit(got[:, 6]).any()


def test_pool_grad_refusals(ctx):
    x, dy, _ = pool_case(("tf", 3, 2, 1), (7, 9), "relu")
    with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, dy) as dd, _canary(ctx, x.shape) as dx:
        # window 4; stride 3; stride > window; padding beyond half the window; a window larger than the map
        for fn, args in ((_lib.pool_tf_grad_nhwc, (4, 2, 1)), (_lib.pool_tf_grad_nhwc, (3, 3, 0)), (_lib.pool_tf_grad_nhwc, (1, 2, 0)),
                         (_lib.maxpool_grad_nhwc, (2, 2, 2)), (_lib.maxpool_grad_nhwc, (9, 2, 0))):
            with pytest.raises(_lib.WscError) as ei:
                fn(ctx, xd.ptr, dd.ptr, 2, 7, 9, 16, args[0], args[1], args[2], dx.ptr)
            assert ei.value.status == _lib.WSC_ERR_INVALID
        ctx.sync()
        assert (dx.to_host() == CANARY).all()


# ---- the whole pass ----------------------------------------------------------------------------------------------------------------
def _pools_key(pools):
    return None if pools is None else tuple(pools)


@functools.lru_cache(maxsize=None)
def model(root, bn, pools, prec):
    """the package's model object at the real widths, one per (stack, BatchNorm, pools, precision) for the module"""
    cls = vgg16_cam.CAM if root == "vgg16" else m7_cam.CAM
    m = cls(None, "voc12", "", 20, None, precision=PRECS[prec], pooling=None if pools is None else list(pools))
    m.load_state_dict(gref.state_dict(root, bn))
    m.eval().cuda(0)
    return m


@functools.lru_cache(maxsize=None)
def run_case(case, prec):
    """One training forward pass and two backward passes of a case on the device, everything downloaded once:
    -> dict(tape {name: array}, feat, grads {name: array}, running {name: array} after this FIRST forward pass of the model, layout)"""
    root, bn, pools, hw = case
    m = model(root, bn, _pools_key(pools), prec)
    ctx, net = m.ctx, m._ensure_net()
    x = gref.net_input(hw)
    stale = m.__dict__.pop("_bn_running", None)  # the running statistics start from the state dict's
    if stale is not None:
        stale.free()
    feat, tape = m.forward_train_dev(x)
    with feat, tape:
        assert ctx.range_status() == 0
        out = {"feat": feat.to_host(), "tape": {e["name"]: tape.entry(e["name"]) for e in tape.entries}, "entries": tape.entries,
               "running": m.bn_running()}
        flat = tape.maps.to_host()
        for e in tape.entries:  # on 256-byte lines, in order, nothing between them but the round-up
            assert e["offset"] % 64 == 0
        dfeat = gref.case_dfeat(case, feat.shape)
        grad = m.cls_grad()
        flats = []
        with _guarded(ctx, dfeat) as dd:
            for _ in range(2):
                with _canary(ctx, (grad.grad_elems,)) as g:
                    grad.backward(B, hw[0], hw[1], tape.maps.ptr, tape.elems, dd.ptr, g.ptr)
                    flats.append(_checked(g, (grad.grad_elems,), "grad"))
            assert np.array_equal(_bits(flats[0]), _bits(flats[1]))  # two calls: identical bits
            with m.backward_dev(tape, DeviceMaps(ctx, dfeat.shape, np.float32, dd.buf)) as g:
                assert np.array_equal(_bits(g.maps.to_host()), _bits(flats[0]))
                out["grads"] = g.to_state_dict()
                one = g.layout[0]["name"]
                assert g[one].shape == (3, 3, 3, 64) and g[one].ptr == g.ptr(one) == g.maps.ptr + 4 * g.layout[0]["offset"]
                assert np.array_equal(g[one].to_host().transpose(3, 2, 0, 1), out["grads"][one])
        # a second forward pass: the same bits in the tape and the features (the running statistics move, nothing reads them)
        feat2, tape2 = m.forward_train_dev(x)
        with feat2, tape2:
            assert np.array_equal(_bits(feat2.to_host()), _bits(out["feat"]))
            flat2 = tape2.maps.to_host()
            for e in tape.entries:
                n = (1 if e["name"].endswith(".stats") else B) * e["Ho"] * e["Wo"] * e["C"]
                assert np.array_equal(_bits(flat[e["offset"]:e["offset"] + n]), _bits(flat2[e["offset"]:e["offset"] + n])), e["name"]
        out["layout"], out["grad_elems"] = grad.layout, grad.grad_elems
    return out


B = gref.B
RUNS = [(c, p) for c in gref.GRAD_CASES for p in ("f32", "f16x3")]


def _run_id(v):
    return gref.case_id(v) if isinstance(v, tuple) else v


@pytest.mark.parametrize("case,prec", RUNS, ids=_run_id)
def test_backward_vs_oracle(case, prec):
    root, bn, pools, hw = case
    sd = gref.state_dict(root, bn)
    res = run_case(case, prec)
    dfeat = gref.case_dfeat(case, res["feat"].shape)
    want = gref.chain_grads(root, sd, res["tape"], dfeat, pools)
    names = gref.param_names(root, sd)
    # one entry per parameter in plain_module_order under state-dict names, torch's shapes, no gaps, no Linear
    assert [e["name"] for e in res["layout"]] == names == list(res["grads"])
    assert all(res["grads"][n].shape == tuple(sd[n].shape) for n in names)
    assert res["grad_elems"] == sum(int(np.prod(sd[n].shape)) for n in names)
    worst = gref.worst_ratio(res["grads"], want)
    print("backward_cls %s %s: worst max|d| / max|g64| %.3e at %s (bound %.3e)" % ((gref.case_id(case), prec) + worst + (64 * gref.R32_CHAIN_CLS,)))
    for n, w in want.items():
        assert np.abs(w).max() > 0, n
        assert np.abs(res["grads"][n].astype(np.float64) - w).max() <= 64 * gref.R32_CHAIN_CLS * np.abs(w).max(), n


@pytest.mark.parametrize("case,prec", RUNS, ids=_run_id)
def test_tape(case, prec):
    """every entry against the float64 op on the entries it read; the running statistics against the oracle's"""
    root, bn, pools, hw = case
    sd = gref.state_dict(root, bn)
    res = run_case(case, prec)
    tape = res["tape"]
    ops = gref.stack_ops(root, sd)
    want_names = ["input"]
    for kind, name, bnk in ops:
        want_names += [name] + ([name + ".bn", name + ".stats"] if bnk else [])
    assert [e["name"] for e in res["entries"]] == want_names
    x = gref.net_input(hw).transpose(0, 2, 3, 1)
    if prec == "f32":
        assert np.array_equal(_bits(tape["input"]), _bits(x))
    else:
        assert (np.abs(tape["input"].astype(np.float64) - x) <= 2.0 ** -22 * np.abs(x) + 2.0 ** -25).all()
    split = (2.0 ** -22, 2.0 ** -25) if prec == "f16x3" else (0.0, 0.0)
    worst = {"conv": 0.0, "bn": 0.0, "stats": 0.0, "running": 0.0}
    prev, n_pool, running = "input", 0, {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)

    for kind, name, bnk in ops:
        got = tape[name].astype(np.float64)
        if kind == "pool":
            ref = gref._nhwc(gref._pool(t(tape[prev]), pools, n_pool))
            assert got.shape == ref.shape and np.array_equal(got, ref), name
            prev, n_pool = name, n_pool + 1
            continue
        w = sd[name + ".weight"]
        ly = nt.Layer(name, "conv", nt.plain_conv(w, sd[name + ".bias"], None, None), (0, nt.NONE, nt.NONE), K=int(np.prod(w.shape[1:])))
        ref, A, S = [v.numpy().transpose(0, 2, 3, 1) for v in ly.fn(t(tape[prev]))]
        bound = nt.asserted_bound(prec, ly, ref, A, S)[0]
        err = np.abs(got - ref)
        assert got.shape == ref.shape and (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        worst["conv"] = max(worst["conv"], float((err / np.maximum(bound, 1e-300)).max()))
        prev = name
        if not bnk:
            continue
        C = got.shape[-1]
        a = tape[name].reshape(-1, C)
        M = a.shape[0]
        gamma, beta = sd[bnk + ".weight"].numpy(), sd[bnk + ".bias"].numpy()
        mean, var, rstd, y64 = gref.bn_train_ref(a, gamma, beta, EPS32)
        b_mean, b_rstd, b_y, dmean, dvar = bn_bounds(a, gamma, mean, var, rstd, y64)
        st = tape[name + ".stats"].astype(np.float64)
        assert st.shape == (C, 2)
        e_m, e_r = np.abs(st[:, 0] - mean), np.abs(st[:, 1] - rstd)  # (a dead channel: mean 0 with the bound 0, exactly)
        assert (e_m <= b_mean).all() and (e_r <= b_rstd).all() and (e_r <= 2.0 ** -23 * rstd).all(), name
        e_st = np.maximum(e_m / np.maximum(b_mean, 1e-300), e_r / b_rstd)
        e_y = np.abs(tape[name + ".bn"].reshape(-1, C).astype(np.float64) - y64)
        b_y = b_y + split[0] * np.abs(y64) + split[1]
        assert (e_y <= b_y).all(), (name, float((e_y / b_y).max()))
        worst["bn"], worst["stats"] = max(worst["bn"], float((e_y / b_y).max())), max(worst["stats"], float(e_st.max()))
        r0 = np.stack([sd[bnk + ".running_mean"].numpy(), sd[bnk + ".running_var"].numpy()]).astype(np.float64)
        want_run = np.stack([KEEP32 * r0[0] + (1 - KEEP32) * mean, KEEP32 * r0[1] + (1 - KEEP32) * var * M / (M - 1)])
        got_run = np.stack([res["running"][bnk + ".running_mean"], res["running"][bnk + ".running_var"]]).astype(np.float64)
        b_run = U * np.abs(want_run) + (1 - KEEP32) * np.stack([dmean, dvar * M / (M - 1)]) + 4 * V * (np.abs(r0) + np.abs(want_run))
        assert (np.abs(got_run - want_run) <= b_run).all(), name
        worst["running"] = max(worst["running"], float((np.abs(got_run - want_run) / b_run).max()))
        prev = name + ".bn"
    assert np.array_equal(_bits(res["feat"]), _bits(tape[prev]))  # feat_dev is the last entry
    print("cls tape %s %s: worst err / bound %s" % (gref.case_id(case), prec, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if prec == "f32" and bn:  # kernel 1 on a taped input writes the taped statistics and the taped output
        name, bnk = next((n, k) for _, n, k in ops if k)
        m = model(root, bn, _pools_key(pools), prec)
        a = tape[name].reshape(-1, tape[name].shape[-1])
        stats, y, _ = run_bn_train(m.ctx, a, sd[bnk + ".weight"].numpy(), sd[bnk + ".bias"].numpy(), None)
        assert np.array_equal(_bits(stats), _bits(tape[name + ".stats"])) and np.array_equal(_bits(y), _bits(tape[name + ".bn"].reshape(a.shape)))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_features_of_a_net_without_batch_norm_are_forward_features(prec):
    case = ("m7", False, gref.KERAS_POOLS, (33, 33))
    res = run_case(case, prec)
    m = model("m7", False, _pools_key(gref.KERAS_POOLS), prec)
    ctx, net = m.ctx, m._ensure_net()
    with DeviceMaps.from_host(ctx, gref.net_input((33, 33))) as xd, _canary(ctx, res["feat"].shape) as fd:
        net.forward_features(xd.ptr, B, 33, fd.ptr)
        assert np.array_equal(_bits(_checked(fd, res["feat"].shape, "feat")), _bits(res["feat"]))


def test_refusals_before_any_launch(ctx):
    """a wrong net, ctx, tape size or gradient size, a keep outside [0, 1], the unbiased variance of one value: WSC_ERR_INVALID, and
    the guard bands and the outputs themselves keep their canaries"""
    case = ("m7", True, None, (40, 24))
    m = model("m7", True, None, "f32")
    mctx, net = m.ctx, m._ensure_net()
    H, W = case[3]
    entries, elems = net.cls_tape_plan(B, H, W)
    h, w = net.cam_size_hw(H, W)
    grad = m.cls_grad()
    with DeviceMaps.from_host(mctx, gref.net_input((H, W))) as xd, _canary(mctx, (elems,)) as tape, _canary(mctx, (B, h, w, 256)) as feat, \
            _canary(mctx, (grad.grad_elems,)) as out, DeviceMaps.from_host(mctx, np.zeros((B, h, w, 256), np.float32)) as dfeat:
        bad = [lambda: net.forward_cls_train(xd.ptr, B, H, W, tape.ptr, elems - 64, feat.ptr),
               lambda: net.forward_cls_train(xd.ptr, B, H, W, tape.ptr, elems, feat.ptr, keep=1.25),
               lambda: net.forward_cls_train(xd.ptr, B, H, W, tape.ptr, elems, feat.ptr, keep=float("nan")),
               lambda: net.forward_cls_train(xd.ptr, B, H, W, tape.ptr + 4, elems, feat.ptr),
               lambda: net.forward_cls_train(xd.ptr, B, H, W, tape.ptr, elems, None),
               lambda: net.forward_cls_train(xd.ptr, 1, 4, 4, tape.ptr, net.cls_tape_plan(1, 4, 4)[1], feat.ptr),  # layer3_p1 sees 1 x 1
               lambda: grad.backward(B, H, W, tape.ptr, elems - 64, dfeat.ptr, out.ptr),
               lambda: grad.backward(B, H, W, tape.ptr, elems, dfeat.ptr, out.ptr, grad_elems=grad.grad_elems - 1),
               lambda: grad.backward(B, H, W, tape.ptr, elems, None, out.ptr),
               lambda: grad.backward(B, H, W, tape.ptr, elems, dfeat.ptr, out.ptr, ctx=ctx)]  # the workspace belongs to the model's stream
        for call in bad:
            with pytest.raises(_lib.WscError) as ei:
                call()
            assert ei.value.status == _lib.WSC_ERR_INVALID
        mctx.sync()
        for buf, shape in ((tape, (elems,)), (feat, (B, h, w, 256)), (out, (grad.grad_elems,))):
            assert (_checked(buf, shape, "refused", written=False) == CANARY).all()  # nothing was launched
        # the Python layer: shapes and objects of another kind
        et = cls_train.ClsTape(DeviceMaps(mctx, (elems,), np.float32, tape.buf), entries, B, H, W)
        with DeviceMaps(mctx, (B, h, w, 255), np.float32) as bad_d:
            for a, b in ((et, bad_d), (et, dfeat.to_host()), (tape, dfeat)):
                with pytest.raises(ValueError):
                    m.backward_dev(a, b)
        for bad_x, kw in ((np.zeros((B, 4, H, W), np.float32), {}), (np.zeros((B, 3, H, W), np.float32), {"bn_keep": 1.5})):
            with pytest.raises(ValueError):
                m.forward_train_dev(bad_x, **kw)
    sd = {k: v.numpy() for k, v in gref.state_dict("m7", True).items()}
    sd.update(m._extra_tensors(m._sd))
    wrong = dict(sd)
    wrong["m7.layer2.0.weight"] = np.zeros((128, 32, 3, 3), np.float32)
    with pytest.raises(_lib.WscError) as ei:
        _lib.ClsGrad(net, wrong)
    assert ei.value.status == _lib.WSC_ERR_SHAPE and "m7.layer2.0" in str(ei.value)
    # any other net has no such tape and no such backward pass
    cam_sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
    cam = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, cam_sd, 20, _lib.PREC_F16)
    try:
        with pytest.raises(_lib.WscError) as ei:
            cam.cls_tape_plan(1, 64, 64)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        with pytest.raises(_lib.WscError) as ei:
            _lib.ClsGrad(cam, cam_sd)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        with DeviceMaps(ctx, (64,), np.float32) as buf, pytest.raises(_lib.WscError) as ei:
            cam.forward_cls_train(buf.ptr, 1, 64, 64, buf.ptr, 64, buf.ptr)
        assert ei.value.status == _lib.WSC_ERR_INVALID
    finally:
        cam.close()


def test_nan_in_the_input_never_leaves_as_finite_gradients():
    """WSC_PREC_F32 carries a NaN through.  The documented outcome is the range status at the next synchronisation (the input door
    raises the flag in every precision); behind it the gradients are looked at all the same: BatchNorm spreads the NaN over every
    channel, so every conv and BatchNorm WEIGHT gradient -- a product with those activations -- is NaN.  (The bias gradients are sums
    of the masked dy, and the mask of a NaN activation is false, NaN > 0: they may be finite, which is why the status is the
    contract.)"""
    case = ("m7", True, None, (40, 24))
    m = model("m7", True, None, "f32")
    ctx = m.ctx
    x = gref.net_input(case[3]).copy()
    x[1, 2, 17, 5] = np.nan
    raised, grads = None, None
    try:
        feat, tape = m.forward_train_dev(x, bn_keep=None)
        with feat, tape, DeviceMaps.from_host(ctx, gref.case_dfeat(case, feat.shape)) as dfeat, m.backward_dev(tape, dfeat) as g:
            try:
                flat = g.maps.to_host()
            except _lib.WscError as e:  # the flag is sticky until cleared; the gradients are looked at all the same
                raised = e.status
                ctx.range_status(clear=True)
                flat = g.maps.to_host()
            grads = {e["name"]: flat[e["offset"]:e["offset"] + e["size"]] for e in g.layout}
    finally:
        ctx.range_status(clear=True)
    print("NaN input: %s" % ("status %d" % raised if raised is not None else "gradients, %d of %d tensors not finite" % (
        sum(1 for v in grads.values() if not np.isfinite(v).all()), len(grads))))
    assert raised == _lib.WSC_ERR_RANGE
    assert not np.isfinite(grads["m7.layer1.0.weight"]).all()  # the first conv reads the NaN itself
    assert all(not np.isfinite(v).all() for n, v in grads.items() if n.endswith(".weight"))


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_grad_step(monkeypatch):
    case = ("vgg16", True, None, (33, 33))
    m = model("vgg16", True, None, "f16x3")
    ctx = m.ctx
    x = gref.net_input(case[3])
    rng = np.random.default_rng(8)
    targets = (rng.random((B, 20)) < 0.3).astype(np.float32)
    loss = cls_train.ClsLoss(ctx, "mean", 20)
    w, bias = m.classifier_params()
    feat, tape = m.forward_train_dev(x)
    with feat, tape:
        want_metrics, head = loss.grad_step(feat, w, bias, targets, np.array([1.0, 2.0], np.float32))
        with head.feat, head.w, head.bias, m.backward_dev(tape, head.feat) as want:
            want_flat, want_head = want.maps.to_host(), [h.to_host() for h in head]
    handed = []
    alloc0 = ctx.alloc

    def alloc(nbytes, pooled=False):
        handed.append(alloc0(nbytes, pooled=pooled))
        return handed[-1]

    monkeypatch.setattr(ctx, "alloc", alloc)
    metrics, head, grads = cls_train.grad_step(m, loss, x, targets, np.array([1.0, 2.0], np.float32))
    monkeypatch.undo()
    with head.feat, head.w, head.bias, grads:
        assert metrics == want_metrics  # to the bits
        assert all(np.array_equal(_bits(a.to_host()), _bits(b)) for a, b in zip(head, want_head))
        assert np.array_equal(_bits(grads.maps.to_host()), _bits(want_flat)) and np.abs(want_flat).max() > 0
        # every buffer of the step but the four results went back
        assert {b.ptr for b in handed if b.ptr is not None} == {grads.maps.ptr, head.feat.ptr, head.w.ptr, head.bias.ptr}
        sd = grads.to_state_dict()
        assert sd["vgg16.layer5.4.weight"].shape == (1024, 1024, 3, 3) and sd["vgg16.layer5.4.bias"].shape == (1024,)
        view = grads["vgg16.layer5.6.weight"]  # the last BatchNorm's weight
        assert view.shape == (1024,) and np.array_equal(_bits(view.to_host()), _bits(sd["vgg16.layer5.6.weight"]))
        with pytest.raises(KeyError):
            grads["vgg16.classifier.0.weight"]
    other = _lib.Context(0)
    try:
        with pytest.raises(ValueError):  # the model keeps a context of its own
            cls_train.grad_step(m, cls_train.ClsLoss(other, "mean", 20), x, targets)
    finally:
        other.close()
    with pytest.raises(ValueError):
        cls_train.grad_step(m, loss, x, targets[:1])
