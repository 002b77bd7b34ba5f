"""GPU: dropout in the SEC / DSRG training step (csrc/seg_dropout.hip; wsc_seg_dropout_f32, wsc_net_forward_seg_train,
wsc_net_backward_seg_drop, wsc_relu_bias_grad_scaled; secdsrg.SegNet.forward_dev(dropout=...), SegTrainer(drop_prob=...)) against
tests/seg_dropout_ref.py, the numpy / torch statement of the project's counter-based contract.

  kernel      wsc_seg_dropout_f32 equals the numpy statement BIT FOR BIT, values and keep bytes, in the vector and the scalar form
  forward     drop_prob = 0: forward_seg_tape's bits.  0.5: every fc6* entry is 0 / exactly twice the undropped entry by its site's
              mask; fc7* is 0 where dropped and, where kept, twice the float64 op on the device's own fc6* entry within twice
              net_trace_ref's per-op bound (the doubling is exact); fc8 within the sum of the branches' per-op bounds
  backward    the device gradients against chain_grads_drop(float64) on the device's own tape, the parent's 64 R32_CHAIN bounds
              (scaling by 2 adds no rounding)
  trainer     SegTrainer(drop_prob=0.5).step is the composition, bit for bit; save / load resumes the random stream
Every device output of the kernel tests has guard bands of CANARY that must survive."""
import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import deeplab_grad_ref as gref
from tests import deeplab_ref as ref
from tests import net_trace_ref as nt
from tests import seg_dropout_ref as dref
from tests import seg_sgd_ref as sgd
from wsscam import _lib, secdsrg
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
CANARY = np.float32(-777.25)
GUARD = 64
PRECS = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the kernel's bits ------------------------------------------------------------------------------------------------------------
def _kernel_input(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10).astype(np.float32)
    special = np.array([-0.0, 1e-41, -3e-45, np.inf, -np.inf, 0.0, 1.17549435e-38, 3.4e38], np.float32)
    at = rng.permutation(n)[:min(n, 2 * special.size)]
    x[at] = np.resize(special, at.size)
    return x


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "off-grid"])
@pytest.mark.parametrize("first", [0, 3, 1 << 34, (1 << 34) + 1], ids=["first0", "first3", "first2p34", "first2p34p1"])
@pytest.mark.parametrize("elems", [1, 3, 4, 5, 4480, 10369, 65537])
def test_kernel_bits(ctx, elems, first, lead):
    """lead = 1: every buffer one float (the keep bytes: one byte) off the 16-byte grid -- the scalar form, as for a `first` that is
    no multiple of 4; lead = 0 with first 0 / 2^34: the 16-byte form with its scalar tail.  -0.0, denormals, inf and the largest
    finite values are among the inputs (3.4e38 / 0.7 overflows to inf: the one fp32 rounding of the contract)."""
    x = _kernel_input(elems, elems + lead)
    band = np.full((GUARD,), CANARY, np.float32)
    kband = np.full((GUARD,), 0xA5, np.uint8)
    for drop_prob, seed, step, site in ((0.0, 5, 0, 0), (0.3, (7 << 32) + 11, 4, 1), (0.5, 5, 1, 7), (0.999, 123456789, 0xFFFFFFFF, 2)):
        want, wkeep = dref.dropout_f32(x, drop_prob, seed, step, site, first)
        with DeviceMaps.from_host(ctx, np.concatenate([band[:lead], x])) as xd, \
                DeviceMaps.from_host(ctx, np.concatenate([band, band[:lead], np.full((elems,), CANARY, np.float32), band])) as yd, \
                DeviceMaps.from_host(ctx, np.concatenate([kband, kband[:lead], np.full((elems,), 0xA5, np.uint8), kband])) as kd:
            assert xd.ptr % 16 == 0 and yd.ptr % 16 == 0 and kd.ptr % 16 == 0  # (GUARD floats / bytes keep the grid)
            _lib.seg_dropout_f32(ctx, xd.ptr + 4 * lead, elems, first, drop_prob, seed, step, site, yd.ptr + 4 * (GUARD + lead),
                                 kd.ptr + GUARD + lead)
            y, k = yd.to_host(), kd.to_host()
        got, gkeep = y[GUARD + lead:GUARD + lead + elems], k[GUARD + lead:GUARD + lead + elems]
        assert (y[:GUARD + lead] == CANARY).all() and (y[GUARD + lead + elems:] == CANARY).all(), "a store outside y"
        assert (k[:GUARD + lead] == 0xA5).all() and (k[GUARD + lead + elems:] == 0xA5).all(), "a store outside keep"
        assert np.array_equal(gkeep, wkeep.astype(np.uint8)), (drop_prob, int((gkeep != wkeep).sum()))
        assert np.array_equal(_bits(got), _bits(want)), (drop_prob, int((_bits(got) != _bits(want)).sum()))
        if drop_prob == 0.0:
            assert np.array_equal(_bits(got), _bits(x))
    # in place, without keep bytes: the same bits
    want, _ = dref.dropout_f32(x, 0.5, 9, 2, 3, first)
    with DeviceMaps.from_host(ctx, np.concatenate([band, band[:lead], x, band])) as xd:
        p = xd.ptr + 4 * (GUARD + lead)
        _lib.seg_dropout_f32(ctx, p, elems, first, 0.5, 9, 2, 3, p)
        y = xd.to_host()
    assert np.array_equal(_bits(y[GUARD + lead:GUARD + lead + elems]), _bits(want))
    assert (y[:GUARD + lead] == CANARY).all() and (y[GUARD + lead + elems:] == CANARY).all()


# ---- 2 / 3. the forward pass ------------------------------------------------------------------------------------------------------
def _tape_dict(tape, flat):
    B = tape.input_shape[0]
    return {e["name"]: flat[e["offset"]:e["offset"] + B * e["Ho"] * e["Wo"] * e["C"]].reshape(B, e["Ho"], e["Wo"], e["C"]) for e in tape.entries}


def _forward(net, xd, dropout):
    """-> (prob, fc8, the flat tape, the tape as a dict) on the host"""
    prob, fc8, tape = net.forward_dev(xd, want_fc8=True, keep=True, dropout=dropout)
    with prob, fc8, tape:
        assert tape.drop_prob == (0.0 if dropout is None else dropout[0])
        flat = tape.to_host()
        return prob.to_host(), fc8.to_host(), flat, _tape_dict(tape, flat)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_forward_at_zero_is_the_tape_pass(ctx, prec):
    """wsc_net_forward_seg_train at drop_prob = 0: wsc_net_forward_seg_tape's prob, fc8 and every tape entry, bit for bit"""
    method, C, hw = "DSRG", 5, (65, 65)
    weights, x = ref.thin_case(method, C, hw)
    net = secdsrg.SegNet(method, weights, C, precision=PRECS[prec], ctx=ctx)
    try:
        with DeviceMaps.from_host(ctx, x) as xd:
            p0, f0, t0, _ = _forward(net, xd, None)
            p1, f1, t1, _ = _forward(net, xd, (0.0, 5, 3))
    finally:
        net.close()
    assert np.array_equal(_bits(p0), _bits(p1)) and np.array_equal(_bits(f0), _bits(f1)) and np.array_equal(_bits(t0), _bits(t1))
    assert np.abs(t0).max() > 0


def _nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_forward_at_half(ctx, method, prec):
    C, hw, seed, step = 5, (65, 65), (3 << 32) + 17, 6
    weights, x = ref.thin_case(method, C, hw)
    net = secdsrg.SegNet(method, weights, C, precision=PRECS[prec], ctx=ctx)
    try:
        with DeviceMaps.from_host(ctx, x) as xd:
            _, _, _, T0 = _forward(net, xd, None)
            _, fc8, _, T1 = _forward(net, xd, (0.5, seed, step))
    finally:
        net.close()
    for name in T0:  # the trunk does not know about dropout
        if name[:2] != "fc":
            assert np.array_equal(_bits(T0[name]), _bits(T1[name])), name
    worst = {"fc7": 0.0, "fc8": 0.0}
    fc8_ref, fc8_bound, fc8_abs = 0.0, 0.0, 0.0
    for k, (sfx, _) in enumerate(gref.branches(method)):
        a6, a7 = T1["fc6" + sfx], T1["fc7" + sfx]
        m6 = dref.keep_mask(a6.shape, 0.5, seed, step, dref.site_of(k, 6))
        m7 = dref.keep_mask(a7.shape, 0.5, seed, step, dref.site_of(k, 7))
        assert 0.45 < m6.mean() < 0.55 and 0.45 < m7.mean() < 0.55
        assert not a6[~m6].any() and not np.signbit(a6[~m6]).any(), "fc6%s: a dropped element is not +0.0" % sfx
        assert np.array_equal(_bits(a6[m6]), _bits(np.float32(2.0) * T0["fc6" + sfx][m6])), "fc6%s: a kept element is not twice the undropped one" % sfx
        assert T0["fc6" + sfx][m6].max() > 0
        assert not a7[~m7].any() and not np.signbit(a7[~m7]).any(), "fc7%s: a dropped element is not +0.0" % sfx
        # fc7 where kept: twice relu(conv(the device's own dropped fc6) + b), within twice the per-op bound
        w7 = nt._d(weights["fc7" + sfx]["w"]).permute(3, 2, 0, 1).contiguous()
        ly = nt.Layer("fc7" + sfx, "conv", nt.plain_conv(w7, weights["fc7" + sfx]["b"], None, None, pad=0), (nt.INPUT, nt.NONE, nt.NONE), K=int(w7.shape[1]))
        r, A, S = [_nhwc(t) for t in ly.fn(_nchw64(a6))]
        bound, _, _ = nt.asserted_bound(prec, ly, r, A, S)
        ratio = float((np.abs(a7.astype(np.float64) - 2.0 * r)[m7] / (2.0 * bound[m7])).max())
        worst["fc7"] = max(worst["fc7"], ratio)
        assert ratio <= 1.0, ("fc7" + sfx, ratio)
        assert (r[m7] > 0).any()
        # fc8: the branches' logits summed in fp32
        w8 = nt._d(weights["fc8" + sfx]["w"]).permute(3, 2, 0, 1).contiguous()
        l8 = nt.Layer("fc8" + sfx, "head", nt.head(w8, weights["fc8" + sfx]["b"]), (nt.INPUT, nt.NONE, nt.NONE), K=int(w8.shape[1]))
        r8, A8, S8 = [_nhwc(t) for t in l8.fn(_nchw64(a7))]
        b8, _, _ = nt.asserted_bound(prec, l8, r8, A8, S8, f32_out=True)
        fc8_ref, fc8_bound, fc8_abs = fc8_ref + r8, fc8_bound + b8, fc8_abs + np.abs(r8) + b8
    nb = len(gref.branches(method))
    fc8_bound = fc8_bound + (nb - 1) * U * fc8_abs  # (the nb - 1 fp32 additions of the sum)
    worst["fc8"] = float((np.abs(fc8.astype(np.float64) - fc8_ref) / fc8_bound).max())
    print("forward at 0.5 %s %s: worst err / bound fc7 %.3f, fc8 %.3f" % (method, prec, worst["fc7"], worst["fc8"]))
    assert worst["fc8"] <= 1.0


@pytest.mark.parametrize("prec", [_lib.PREC_F16, _lib.PREC_BF16, _lib.PREC_BF16X3], ids=["f16", "bf16", "bf16x3"])
def test_forward_at_half_other_precisions(ctx, prec):
    """the one-plane and the bfloat16 forms of the kernel: the fc6* / fc7* entries are +0.0 by their site's mask, and a kept fc6*
    element is exactly twice the undropped one (a doubling is exact in every 16-bit format short of its ceiling)"""
    method, C, hw, seed, step = "DSRG", 5, (65, 65), 31, 1
    weights, x = ref.thin_case(method, C, hw)
    net = secdsrg.SegNet(method, weights, C, precision=prec, ctx=ctx)
    try:
        with DeviceMaps.from_host(ctx, x) as xd:
            _, _, _, T0 = _forward(net, xd, None)
            _, _, _, T1 = _forward(net, xd, (0.5, seed, step))
    finally:
        net.close()
    for k, (sfx, _) in enumerate(gref.branches(method)):
        for layer in (6, 7):
            a = T1["fc%d%s" % (layer, sfx)]
            m = dref.keep_mask(a.shape, 0.5, seed, step, dref.site_of(k, layer))
            assert not a[~m].any() and not np.signbit(a[~m]).any() and a[m].max() > 0
        m6 = dref.keep_mask(T1["fc6" + sfx].shape, 0.5, seed, step, dref.site_of(k, 6))
        assert np.array_equal(_bits(T1["fc6" + sfx][m6]), _bits(np.float32(2.0) * T0["fc6" + sfx][m6]))


# ---- 4. the scaled mask step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0, float(np.float32(1.0) / np.float32(0.7))], ids=["2", "1/0.7"])
@pytest.mark.parametrize("M, C", [(1, 64), (70, 64), (81, 1024)])
def test_relu_bias_grad_scaled(ctx, M, C, scale):
    rng = np.random.default_rng(M + C)
    y = (np.maximum(rng.integers(-8, 9, (M, C)), 0) / 4.0).astype(np.float32)
    dy = (1e-3 * rng.standard_normal((M, C))).astype(np.float32)
    dy[0, 0] = -0.0
    want = np.where(y > 0, np.float32(dy * np.float32(scale)), np.float32(0.0)).astype(np.float32)
    n = M * C
    band = np.full((GUARD,), CANARY, np.float32)
    with DeviceMaps.from_host(ctx, y) as yd, DeviceMaps.from_host(ctx, dy) as gd, \
            DeviceMaps.from_host(ctx, np.full((n + GUARD,), CANARY, np.float32)) as dz, DeviceMaps.from_host(ctx, np.full((C + GUARD,), CANARY, np.float32)) as db:
        _lib.relu_bias_grad_scaled(ctx, yd.ptr, gd.ptr, M, C, scale, dz.ptr, db.ptr)
        z, b = dz.to_host(), db.to_host()
        assert np.array_equal(z[n:], band) and np.array_equal(b[C:], band)
        assert np.array_equal(_bits(z[:n].reshape(M, C)), _bits(want))  # float32(dy scale) or +0.0, to the bits
        w64 = want.astype(np.float64)
        errb = np.abs(b[:C].astype(np.float64) - w64.sum(0))
        assert (errb <= (M + 2) * U * np.abs(w64).sum(0)).all()
        # scale 1.0f: the unscaled entry's bits
        _lib.relu_bias_grad_scaled(ctx, yd.ptr, gd.ptr, M, C, 1.0, dz.ptr, db.ptr)
        z1, b1 = dz.to_host(), db.to_host()
        _lib.relu_bias_grad(ctx, yd.ptr, gd.ptr, M, C, dz.ptr, db.ptr)
        assert np.array_equal(_bits(z1), _bits(dz.to_host())) and np.array_equal(_bits(b1), _bits(db.to_host()))


# ---- 5 / 6. the backward pass -------------------------------------------------------------------------------------------------------
def _layer_grads(flat, layout):
    out = {}
    for layer, e in layout.items():
        nw = e["k"] * e["k"] * e["Cin"] * e["Cout"]
        out[layer] = {"w": flat[e["w_off"]:e["w_off"] + nw].reshape(e["k"], e["k"], e["Cin"], e["Cout"]), "b": flat[e["b_off"]:e["b_off"] + e["Cout"]]}
    return out


def _backward_drop(ctx, method, C, weights, x, prec, dfc8_of, drop):
    """-> (device gradients {layer: {'w', 'b'}}, chain_grads_drop(float64) on the device's own tape, the flat gradient, the tape)"""
    net = secdsrg.SegNet(method, weights, C, precision=PRECS[prec], ctx=ctx)
    try:
        prob, tape = net.forward_dev(x, keep=True, dropout=drop)
        with prob, tape:
            dfc8 = dfc8_of(prob.shape)
            with net.backward_dev(tape, dfc8) as grads:
                flat = grads.maps.to_host()
                with net.backward_dev(tape, dfc8) as again:  # two calls: the same bits
                    assert np.array_equal(_bits(flat), _bits(again.maps.to_host()))
                got = _layer_grads(flat, grads.layout)
            tflat = tape.to_host()
            want = dref.chain_grads_drop(method, weights, _tape_dict(tape, tflat), dfc8, drop[0], torch.float64)
    finally:
        net.close()
    return got, want, flat, tflat


def _assert_grads(got, want, method, bound, what):
    assert set(got) == set(ref.layer_names(method))
    ratios = gref.layer_ratio(got, want)
    layer = max(ratios, key=lambda l: max(ratios[l]))
    print("backward_seg_drop %s: worst max|d| / max|g64| = %.3e at %s (bound %.3e)" % (what, max(ratios[layer]), layer, bound))
    for name, (rw, rb) in ratios.items():
        assert np.abs(want[name]["w"]).max() > 0 and np.abs(want[name]["b"]).max() > 0, name
        assert rw <= bound and rb <= bound, (name, rw, rb)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("case", [("SEC", 5, (65, 65)), ("DSRG", 5, (65, 65)), ("DSRG", 21, (64, 48))], ids=lambda c: "%s-%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1]))
def test_backward_end_to_end_at_half(ctx, case, prec):
    """wsc_net_backward_seg_drop on the device's own dropped tape against chain_grads_drop(float64) on that tape: per layer
    max|d| <= 64 R32_CHAIN max|g64| = 1.33e-4, the parent's bound (scaling by 2 adds no rounding).  Worst measured ratio over the six
    cases: 1.56e-6, conv1_2 of ("DSRG", 21, (64, 48)) in both precisions (SEC 1.40e-6, DSRG 5 classes 1.01e-6)."""
    method, C, hw = case
    weights, x = ref.thin_case(method, C, hw)

    def dfc8_of(shape):
        rng = np.random.default_rng(900 + 3 * C + hw[1] + (1 if method == "SEC" else 0))
        return (1e-3 * rng.standard_normal(shape)).astype(np.float32)

    got, want, _, _ = _backward_drop(ctx, method, C, weights, x, prec, dfc8_of, (0.5, 41, 2))
    _assert_grads(got, want, method, 64 * gref.R32_CHAIN, "%s %s" % (case, prec))


def test_backward_end_to_end_at_half_full_width(ctx):
    """the real widths (fc 1024, 21 classes): DSRG, 65 x 65, B = 1, f16x3; bound 64 R32_CHAIN_FULL = 9.86e-5, measured 3.10e-6 at
    conv2_1"""
    case = ("DSRG", 21, (65, 65), 1)
    weights, x = gref.full_case(case)
    got, want, _, _ = _backward_drop(ctx, "DSRG", 21, weights, x, "f16x3", lambda shape: gref.full_dfc8(case, shape), (0.5, 41, 2))
    _assert_grads(got, want, "DSRG", 64 * gref.R32_CHAIN_FULL, "full width f16x3")


def test_same_seed_and_step_reproduce_another_step_does_not(ctx):
    method, C, hw = "DSRG", 5, (65, 65)
    weights, x = ref.thin_case(method, C, hw)

    def dfc8_of(shape):
        return (1e-3 * np.random.default_rng(5).standard_normal(shape)).astype(np.float32)

    _, _, g0, t0 = _backward_drop(ctx, method, C, weights, x, "f16x3", dfc8_of, (0.5, 41, 2))
    _, _, g1, t1 = _backward_drop(ctx, method, C, weights, x, "f16x3", dfc8_of, (0.5, 41, 2))
    _, _, g2, t2 = _backward_drop(ctx, method, C, weights, x, "f16x3", dfc8_of, (0.5, 41, 3))
    assert np.array_equal(_bits(g0), _bits(g1)) and np.array_equal(_bits(t0), _bits(t1))
    assert not np.array_equal(_bits(t0), _bits(t2)) and not np.array_equal(_bits(g0), _bits(g2))


# ---- 7. the trainer -------------------------------------------------------------------------------------------------------------------
def _step_case(method, C=5):
    weights, x = ref.thin_case(method, C, (65, 65))
    rng = np.random.default_rng(77)
    cues = (rng.random((2, 9, 9, C)) < 0.2).astype(np.float32)
    tags = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 1]], np.float32)
    return weights, x, cues, tags


def _trainer_step(tr, x, cues, tags):
    losses, new_cues = tr.step(x, cues, tags, MEAN, CRF_CFG)
    new_cues.free()
    return losses


@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_trainer_step_with_dropout_is_the_composition(ctx, method, tmp_path):
    """SegTrainer(drop_prob=0.5): every step equals a fresh SegNet from params_host(), grad_step_dev(dropout=(0.5, seed, calls)) and
    tests/seg_sgd_ref.py, bit for bit; save after step 1, load, step 2 = two uninterrupted steps."""
    C, seed = 5, (9 << 32) + 2024
    weights, x, cues, tags = _step_case(method)
    layout, n = sgd.layout_of(method, weights)
    segs = sgd.segments(layout)
    wd, mo = 5e-4, 0.9
    tr = secdsrg.SegTrainer(method, weights, C, ctx=ctx, drop_prob=0.5, seed=seed)
    tr2 = plain = None
    try:
        params, mom = weights, np.zeros(n, np.float32)
        path = str(tmp_path / "trainer.npy")
        for update in range(2):
            p = sgd.flatten(layout, n, params)
            calls = tr.calls
            assert calls == update
            got_l = _trainer_step(tr, x, cues, tags)
            net = secdsrg.SegNet(method, params, C, ctx=ctx)
            try:
                want_l, grads, new_cues = net.grad_step_dev(x, cues, tags, MEAN, CRF_CFG, dropout=(0.5, seed, calls))
                with grads, new_cues:
                    g = sgd.flatten(layout, n, grads.to_host())
            finally:
                net.close()
            assert {k: got_l[k] for k in want_l} == want_l, update
            acc = sgd.accumulate(segs, p, g, np.zeros(n, np.float32), wd, 1)
            p, acc, mom = sgd.apply(p, acc, mom, sgd.lr_at(0), mo, True)
            assert np.array_equal(_bits(tr.params.to_host()), _bits(p)), (update, int((_bits(tr.params.to_host()) != _bits(p)).sum()))
            assert np.array_equal(_bits(tr.mom.to_host()), _bits(mom))
            params = tr.params_host()
            if update == 0:
                tr.save(path)
                first_losses = got_l
        saved = np.load(path, allow_pickle=True).item()["__step__"]
        assert saved["seed"] == seed and saved["drop_prob"] == 0.5 and saved["calls"] == 1
        tr2 = secdsrg.SegTrainer.load(path, method, C, ctx=ctx)
        assert (tr2.calls, tr2.seed, tr2.drop_prob) == (1, seed, 0.5)
        lb = _trainer_step(tr2, x, cues, tags)
        assert lb == got_l
        for name in ("params", "mom", "accum"):
            assert np.array_equal(_bits(getattr(tr, name).to_host()), _bits(getattr(tr2, name).to_host())), name
        # dropout is in the step: the same first step without it gives other losses; a file without the fields loads as 0
        plain = secdsrg.SegTrainer(method, weights, C, ctx=ctx)
        assert (plain.drop_prob, plain.seed) == (0.0, 0)
        assert _trainer_step(plain, x, cues, tags) != first_losses
        d = np.load(path, allow_pickle=True).item()
        d["__step__"] = {"calls": 1, "lr": float(tr.lr)}
        with open(path, "wb") as fh:
            np.save(fh, d, allow_pickle=True)
        plain.close()
        plain = secdsrg.SegTrainer.load(path, method, C, ctx=ctx)
        assert (plain.calls, plain.seed, plain.drop_prob) == (1, 0, 0.0)
    finally:
        for t in (tr, tr2, plain):
            if t is not None:
                t.close()


# ---- 8. the range flag ---------------------------------------------------------------------------------------------------------------
def test_doubled_activation_at_halfs_ceiling_raises_range(ctx):
    """A thin f16x3 SEC net whose fc6 bias puts fc6's outputs in (32752, 65504): clean at drop_prob = 0, WSC_ERR_RANGE once at 0.5
    (a kept element doubles past 65504 and the stored half saturates), and the net is usable afterwards."""
    method, C, hw = "SEC", 5, (65, 65)
    weights, x = ref.thin_case(method, C, hw)
    weights = {l: {"w": e["w"].copy(), "b": e["b"].copy()} for l, e in weights.items()}
    weights["fc6"]["b"][:] = 48000.0
    weights["fc7"]["w"] *= np.float32(1e-4)  # (fc7 itself stays far inside the range)
    net = secdsrg.SegNet(method, weights, C, precision=_lib.PREC_F16X3, ctx=ctx)
    try:
        with DeviceMaps.from_host(ctx, x) as xd:
            _, _, _, T0 = _forward(net, xd, None)
            assert 32752 < T0["fc6"].min() and T0["fc6"].max() < 65504
            with pytest.raises(_lib.WscError) as ei:
                net.forward_dev(xd, keep=True, dropout=(0.5, 1, 0))
            assert ei.value.status == _lib.WSC_ERR_RANGE
            _, _, _, T1 = _forward(net, xd, None)  # reported once: the flag went with the report
            assert np.array_equal(_bits(T0["fc6"]), _bits(T1["fc6"]))
    finally:
        net.close()


# ---- 9. errors before any launch -----------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(ctx):
    C = 5
    weights, x = ref.thin_case("DSRG", C, (65, 65))
    net = secdsrg.SegNet("DSRG", weights, C, precision=_lib.PREC_F32, ctx=ctx)
    cam = None
    try:
        entries, elems = net.net.seg_tape_plan(2, 65, 65)
        sg = net._ensure_grad()
        canary = np.full((elems,), CANARY, np.float32)
        gcanary = np.full((sg.grad_elems,), CANARY, np.float32)
        small = np.full((64,), CANARY, np.float32)
        with DeviceMaps.from_host(ctx, canary) as tape, DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, np.full((2, 9, 9, C), CANARY, np.float32)) as prob, \
                DeviceMaps.from_host(ctx, gcanary) as grad, DeviceMaps.from_host(ctx, small) as a, DeviceMaps.from_host(ctx, small) as b:
            def fwd(drop_prob=0.5, step=0, tape_ptr=tape.ptr, n=elems, x_ptr=xd.ptr, prob_ptr=prob.ptr):
                return lambda: net.net.forward_seg_train(x_ptr, 2, 65, 65, drop_prob, 1, step, tape_ptr, n, prob_ptr)

            def bwd(drop_prob=0.5, tape_ptr=tape.ptr, n=elems, g_ptr=grad.ptr, d_ptr=prob.ptr, ge=None):
                return lambda: sg.backward_drop(2, 65, 65, tape_ptr, n, d_ptr, g_ptr, drop_prob, grad_elems=ge)

            def ker(drop_prob=0.5, step=0, x_ptr=a.ptr, y_ptr=b.ptr, n=64, first=0, site=0):
                return lambda: _lib.seg_dropout_f32(ctx, x_ptr, n, first, drop_prob, 1, step, site, y_ptr)

            calls = [fwd(drop_prob=-0.1), fwd(drop_prob=1.0), fwd(drop_prob=float("nan")), fwd(step=1 << 32), fwd(step=-1),
                     fwd(tape_ptr=None), fwd(x_ptr=None), fwd(prob_ptr=None), fwd(n=elems - 64),
                     bwd(drop_prob=-0.1), bwd(drop_prob=1.0), bwd(drop_prob=float("nan")), bwd(tape_ptr=None), bwd(g_ptr=None), bwd(d_ptr=None),
                     bwd(n=elems - 64), bwd(ge=sg.grad_elems - 1),
                     ker(drop_prob=-0.1), ker(drop_prob=1.0), ker(drop_prob=float("nan")), ker(step=1 << 32), ker(x_ptr=None), ker(y_ptr=None),
                     ker(n=0), ker(first=-4), ker(site=-1),
                     lambda: _lib.relu_bias_grad_scaled(ctx, a.ptr, a.ptr, 1, 64, 0.5, b.ptr, b.ptr),
                     lambda: _lib.relu_bias_grad_scaled(ctx, a.ptr, a.ptr, 1, 64, float("nan"), b.ptr, b.ptr),
                     lambda: _lib.relu_bias_grad_scaled(ctx, a.ptr, None, 1, 64, 2.0, b.ptr, b.ptr)]
            for i, call in enumerate(calls):
                with pytest.raises(_lib.WscError) as ei:
                    call()
                assert ei.value.status == _lib.WSC_ERR_INVALID, i
            for d, want in ((tape, canary), (grad, gcanary), (a, small), (b, small)):
                assert np.array_equal(_bits(d.to_host()), _bits(want))  # nothing was launched
            assert (prob.to_host() == CANARY).all()
            with pytest.raises(ValueError):
                net.forward_dev(xd, dropout=(0.5, 1, 0))  # dropout= without keep=True
        with pytest.raises(ValueError):
            secdsrg.SegTrainer("DSRG", weights, C, ctx=ctx, drop_prob=1.0)
        # a net that is no DeepLab net
        sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
        cam = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, sd, 20, _lib.PREC_F16)
        with DeviceMaps.from_host(ctx, small) as t:
            with pytest.raises(_lib.WscError) as ei:
                cam.forward_seg_train(t.ptr, 1, 65, 65, 0.5, 1, 0, t.ptr, 64, t.ptr)
            assert ei.value.status == _lib.WSC_ERR_INVALID
            assert (t.to_host() == CANARY).all()
    finally:
        net.close()
        if cam is not None:
            cam.close()
