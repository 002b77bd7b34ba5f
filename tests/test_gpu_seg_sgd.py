"""GPU: the update half of a SEC / DSRG training step (csrc/sgd.hip, csrc/repack.hip; wsc_seg_sgd_accumulate, wsc_seg_sgd_apply,
wsc_net_seg_load_params of csrc/net.hip; secdsrg.SegNet.load_params_dev, secdsrg.SegTrainer).

  optimiser   accumulate + apply on a thin net's whole flat buffer against tests/seg_sgd_ref.py in float32, BIT FOR BIT (param,
              accum, mom); loss["l2"] against the float64 sum to 2^-23 relative (one final rounding; the double sum's own error is
              below 1e-8 of that); a repeated call gives the same bits
  repack      a SegNet created from W0 that load_params_dev's the flat form of W1 computes, forward and backward, the bits of a
              SegNet created from W1 -- every precision, both methods, W1 with the packing's edge cases
  step        SegTrainer.step is the composition: a fresh SegNet from the previous host parameters, grad_step_dev, SegGrads.to_host,
              seg_sgd_ref in float32 -- bit for bit after every update
Every device buffer the optimiser writes has GUARD floats of CANARY behind it that must survive."""
import numpy as np
import pytest

from oracle import cnn_ref
from tests import deeplab_grad_ref as gref
from tests import deeplab_ref as ref
from tests import seg_sgd_ref as sgd
from wsscam import _lib, secdsrg
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
CANARY = np.float32(-777.25)
GUARD = 256  # floats of CANARY behind every device output
PRECS = {"f16x3": _lib.PREC_F16X3, "f32": _lib.PREC_F32, "f16": _lib.PREC_F16, "bf16x3": _lib.PREC_BF16X3}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(ctx, values, lead=0):
    """`values` on the device behind `lead` and in front of GUARD floats of CANARY"""
    return DeviceMaps.from_host(ctx, np.concatenate([np.full((lead,), CANARY, np.float32), values, np.full((GUARD,), CANARY, np.float32)]))


def _body(buf, n, what, lead=0):
    """the n floats of a _guarded buffer, the bands around them untouched"""
    flat = buf.to_host()
    assert flat.size == lead + n + GUARD
    assert (flat[:lead] == CANARY).all() and (flat[lead + n:] == CANARY).all(), what + ": a store outside the buffer"
    return flat[lead:lead + n].copy()


# ---- 1. the optimiser's bits -------------------------------------------------------------------------------------------------------
def _sgd_inputs(n, segs, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    g[rng.integers(0, n, 50)] = 0.0
    g[rng.integers(0, n, 50)] = np.float32(1e-41) * rng.integers(-9, 10, 50).astype(np.float32)  # denormals
    g[rng.integers(0, n, 5)] = -0.0
    _, a, b, _, _ = segs[8]
    g[a:b] = 0.0  # one segment all zero
    acc = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    mom = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    return p, g, acc, mom


def _run_sgd(ctx, sg, p, g, acc, mom, wd, accum_num, clear, want_l2=True, lead=0):
    """accumulate then apply on guarded copies -> (param, accum after accumulate, accum, mom, l2 or None)"""
    n = p.size
    with _guarded(ctx, p, lead) as pd, _guarded(ctx, g, lead) as gd, _guarded(ctx, acc, lead) as ad, _guarded(ctx, mom, lead) as md, \
            _guarded(ctx, np.full((1,), CANARY, np.float32)) as l2:
        at = lambda d: d.ptr + 4 * lead
        sg.sgd_accumulate(at(pd), at(gd), at(ad), wd, accum_num, l2.ptr if want_l2 else None)
        acc1 = _body(ad, n, "accum", lead)
        assert np.array_equal(_bits(_body(pd, n, "param", lead)), _bits(p)) and np.array_equal(_bits(_body(gd, n, "grad", lead)), _bits(g))
        sg.sgd_apply(at(pd), at(ad), at(md), np.float32(1e-4), np.float32(0.9), clear)
        out = (_body(pd, n, "param", lead), acc1, _body(ad, n, "accum", lead), _body(md, n, "mom", lead), _body(l2, 1, "l2")[0])
        assert np.array_equal(_bits(_body(gd, n, "grad", lead)), _bits(g))
    return out if want_l2 else out[:4] + (None,)


@pytest.mark.parametrize("C", [5, 21])
@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_sgd_bits(ctx, method, C):
    weights = ref.random_weights(method, C, 64, 128, seed=3 + C)
    net = secdsrg.SegNet(method, weights, C, precision=_lib.PREC_F32, ctx=ctx)
    try:
        sg = net._ensure_grad()
        layout, n = sgd.layout_of(method, weights)
        assert sg.layout == layout and sg.grad_elems == n  # the reference's table is the library's layout
        assert np.array_equal(net.flat_params(weights), sgd.flatten(layout, n, weights))
        segs = sgd.segments(layout)
        if method == "DSRG":  # behind fc8_1's bias the offsets are odd: segment boundaries inside a 16-byte vector
            assert any(a % 2 for _, a, _, _, _ in segs)
        else:  # the buffer ends inside one
            assert n % 4
        p, g, acc, mom = _sgd_inputs(n, segs, 40 + C)
        l2_64 = sgd.l2(segs, p)
        first = None
        for wd in (0.0, 5e-4):
            for accum_num in (1, 3):
                for clear in (True, False):
                    got = _run_sgd(ctx, sg, p, g, acc, mom, wd, accum_num, clear)
                    acc_w = sgd.accumulate(segs, p, g, acc, wd, accum_num)
                    p_w, acc2_w, mom_w = sgd.apply(p, acc_w, mom, 1e-4, 0.9, clear)
                    for name, a, b in zip(("param", "accum after accumulate", "accum", "mom"), got[:4], (p_w, acc_w, acc2_w, mom_w)):
                        assert np.array_equal(_bits(a), _bits(b)), (name, wd, accum_num, clear, int((_bits(a) != _bits(b)).sum()))
                    rel = abs(float(got[4]) - l2_64) / l2_64
                    assert rel <= 2.0 ** -23, rel
                    if first is None:
                        first = (wd, accum_num, clear, got)
                        print("sgd %s C=%d: %d floats, l2 %.6e, |l2 - float64| / l2 = %.3e (bound %.3e)" % (method, C, n, got[4], rel, 2.0 ** -23))
        wd, accum_num, clear, want = first
        again = _run_sgd(ctx, sg, p, g, acc, mom, wd, accum_num, clear)  # the same calls again: the same bits, l2 included
        no_l2 = _run_sgd(ctx, sg, p, g, acc, mom, wd, accum_num, clear, want_l2=False)  # l2_dev = NULL: the other outputs unchanged
        shifted = _run_sgd(ctx, sg, p, g, acc, mom, wd, accum_num, clear, lead=1)  # buffers off the 16-byte grid: the scalar form
        for other in (again, no_l2, shifted):
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(want[:4], other[:4]))
        assert _bits(np.float32(again[4])) == _bits(np.float32(want[4])) and no_l2[4] is None
        assert abs(float(shifted[4]) - l2_64) / l2_64 <= 2.0 ** -23
    finally:
        net.close()


# ---- 2. the repack equals creation ---------------------------------------------------------------------------------------------------
def _edge_weights(method, C, base):
    """a copy of `base` with the packing's edge cases in conv1_1, a trunk layer, an fc6, an fc7 and an fc8: per layer an output
    channel of zeros, one whose maximum is 1e-40, one whose maximum is a power of two, one just below it, one whose maximum is
    negative, one with magnitudes spread over 2^20"""
    rng = np.random.default_rng(5)
    out = {l: {"w": e["w"].copy(), "b": e["b"].copy()} for l, e in base.items()}
    sfx = "" if method == "SEC" else "_3"
    for layer in dict.fromkeys(("conv1_1", "conv3_2", "fc6" + sfx, "fc7" + sfx, "fc8" + sfx, "fc8" + ("" if method == "SEC" else "_1"))):
        w = out[layer]["w"]
        cols = w.reshape(-1, w.shape[3])  # (a view: rows = the k k Cin weights of an output channel)
        c = 5 if w.shape[3] > 5 else 4  # (a five-class fc8: the spread shares the channel of the negative maximum)
        cols[:, c] *= (2.0 ** -(20 * rng.random(cols.shape[0]))).astype(np.float32)
        cols[:, 0] = 0.0
        cols[:, 1] *= np.float32(1e-40) / np.abs(cols[:, 1]).max()
        cols[:, 2] = np.clip(cols[:, 2], -0.1, 0.1)
        cols[3, 2] = np.float32(2.0 ** -3)
        cols[:, 3] = np.clip(cols[:, 3], -0.1, 0.1)
        cols[5, 3] = np.nextafter(np.float32(2.0 ** -3), np.float32(0))
        cols[7, 4] = -2.0 * np.abs(cols[:, 4]).max()
        assert np.abs(cols[:, 1]).max() <= np.float32(1.0001e-40) and np.abs(cols[:, 1]).max() > 0 and cols[:, 4].min() == -np.abs(cols[:, 4]).max()
    return out


def _forward_backward_bits(net, x, dfc8):
    prob, fc8, tape = net.forward_dev(x, want_fc8=True, keep=True)
    with prob, fc8, tape:
        with net.backward_dev(tape, dfc8) as grads:
            return [_bits(d.to_host()) for d in (prob, fc8, tape, grads.maps)]


def _check_repack(ctx, method, C, prec, w0, w1, inputs):
    a = secdsrg.SegNet(method, w0, C, precision=prec, ctx=ctx)
    b = None
    try:
        shapes = {hw: (x.shape[0],) + tuple(a.map_size(*hw)) + (C,) for hw, x in inputs.items()}
        dfc8 = {hw: (1e-3 * np.random.default_rng(60 + hw[1]).standard_normal(shapes[hw])).astype(np.float32) for hw in inputs}
        hw0 = next(iter(inputs))
        before = _forward_backward_bits(a, inputs[hw0], dfc8[hw0])
        a.load_params_dev(a.flat_params(w0))  # its own weights: nothing changes
        for u, v in zip(before, _forward_backward_bits(a, inputs[hw0], dfc8[hw0])):
            assert np.array_equal(u, v)
        with DeviceMaps.from_host(ctx, a.flat_params(w1)) as flat:  # a DeviceMaps is read in place
            a.load_params_dev(flat)
        b = secdsrg.SegNet(method, w1, C, precision=prec, ctx=ctx)
        for hw, x in inputs.items():
            got, want = _forward_backward_bits(a, x, dfc8[hw]), _forward_backward_bits(b, x, dfc8[hw])
            for name, u, v in zip(("prob", "fc8", "tape", "gradients"), got, want):
                assert np.array_equal(u, v), (name, hw, int((u != v).sum()), u.size)
            assert not np.array_equal(got[1], before[1]) or hw != hw0  # the weights did change
    finally:
        a.close()
        if b is not None:
            b.close()


@pytest.mark.parametrize("prec", list(PRECS), ids=list(PRECS))
@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_repack_equals_creation(ctx, method, prec):
    C = 5
    w0 = ref.random_weights(method, C, 64, 128, seed=21)
    w1 = _edge_weights(method, C, ref.random_weights(method, C, 64, 128, seed=22))
    inputs = {hw: ref.net_input(2, hw[0], hw[1], 70 + hw[1]) for hw in ((65, 65), (64, 48))}
    _check_repack(ctx, method, C, PRECS[prec], w0, w1, inputs)


def test_repack_equals_creation_full_width(ctx):
    """the real widths (128-row CoutPad tiles, Kw = 9 x 512, fc 1024, 21 classes): DSRG, 65 x 65, B = 1, f16x3"""
    w0 = gref.full_weights("DSRG", 21)
    rng = np.random.default_rng(23)
    w1 = {l: {"w": (e["w"] * (1 + 0.25 * rng.standard_normal(e["w"].shape))).astype(np.float32),
              "b": (e["b"] + 0.01 * rng.standard_normal(e["b"].shape)).astype(np.float32)} for l, e in w0.items()}
    _check_repack(ctx, "DSRG", 21, _lib.PREC_F16X3, w0, w1, {(65, 65): ref.net_input(1, 65, 65, 12)})


# ---- 3. the step is the composition ----------------------------------------------------------------------------------------------------
def _step_case(method, C=5):
    weights, x = ref.thin_case(method, C, (65, 65))
    rng = np.random.default_rng(77)
    cues = (rng.random((2, 9, 9, C)) < 0.2).astype(np.float32)
    tags = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 1]], np.float32)
    return weights, x, cues, tags


def _fresh_grad_step(ctx, method, C, params, x, cues, tags):
    """the path without the trainer: a SegNet created from host parameters, grad_step_dev, the gradients on the host, flat"""
    net = secdsrg.SegNet(method, params, C, ctx=ctx)
    try:
        losses, grads, new_cues = net.grad_step_dev(x, cues, tags, MEAN, CRF_CFG)
        with grads, new_cues:
            layout, n = sgd.layout_of(method, params)
            return losses, sgd.flatten(layout, n, grads.to_host())
    finally:
        net.close()


def _trainer_step(tr, x, cues, tags, **kw):
    losses, new_cues = tr.step(x, cues, tags, MEAN, CRF_CFG, **kw)
    new_cues.free()
    return losses


@pytest.mark.parametrize("accum_num", [1, 2])
@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_step_is_the_composition(ctx, method, accum_num, tmp_path):
    C = 5
    weights, x, cues, tags = _step_case(method)
    layout, n = sgd.layout_of(method, weights)
    segs = sgd.segments(layout)
    wd, mo = 5e-4, 0.9
    tr = secdsrg.SegTrainer(method, weights, C, ctx=ctx, accum_num=accum_num)
    tr2 = None
    try:
        assert tr.layout == layout and [tr.lr_at(e) for e in (0, 3.99, 4, 8.5)] == [sgd.lr_at(e) for e in (0, 3.99, 4, 8.5)]
        params, mom = weights, np.zeros(n, np.float32)
        for update in range(2):
            p = sgd.flatten(layout, n, params)
            acc = np.zeros(n, np.float32)
            for call in range(accum_num):
                got_l = _trainer_step(tr, x, cues, tags, epoch=0 if update == 0 and call == 0 else None)
                want_l, g = _fresh_grad_step(ctx, method, C, params, x, cues, tags)
                acc = sgd.accumulate(segs, p, g, acc, wd, accum_num)
                l2_64 = sgd.l2(segs, p)
                assert {k: got_l[k] for k in want_l} == want_l, (update, call)  # the net computes with the updated weights, to the bits
                assert abs(got_l["l2"] - l2_64) <= 2.0 ** -23 * l2_64 and got_l["total"] == got_l["norm"] + wd * got_l["l2"]
                if call + 1 < accum_num:  # no update yet: the parameters stand
                    assert np.array_equal(_bits(tr.params.to_host()), _bits(p))
            p, acc, mom = sgd.apply(p, acc, mom, sgd.lr_at(0), mo, True)
            assert np.array_equal(_bits(tr.params.to_host()), _bits(p)), (update, int((_bits(tr.params.to_host()) != _bits(p)).sum()))
            assert np.array_equal(_bits(tr.mom.to_host()), _bits(mom)) and not tr.accum.to_host().any()
            params = tr.params_host()
            assert np.array_equal(_bits(sgd.flatten(layout, n, params)), _bits(p)) and params["fc7" + ("" if method == "SEC" else "_3")]["w"].shape == (1, 1, 128, 128)
            print("step %s accum_num=%d update %d: norm %.6f l2 %.6f, max |param - start| %.3e"
                  % (method, accum_num, update, got_l["norm"], got_l["l2"], np.abs(p - sgd.flatten(layout, n, weights)).max()))
        if accum_num == 1:  # save -> load -> one more step = an uninterrupted third step
            path = str(tmp_path / "trainer.npy")
            tr.save(path)
            saved = np.load(path, allow_pickle=True).item()
            assert set(ref.layer_names(method)) <= set(saved) and np.array_equal(saved["conv1_1"]["w"], params["conv1_1"]["w"])
            tr2 = secdsrg.SegTrainer.load(path, method, C, ctx=ctx)
            assert tr2.calls == tr.calls and tr2.lr == tr.lr
            la, lb = _trainer_step(tr, x, cues, tags), _trainer_step(tr2, x, cues, tags)
            assert la == lb
            for name in ("params", "mom", "accum"):
                assert np.array_equal(_bits(getattr(tr, name).to_host()), _bits(getattr(tr2, name).to_host())), name
            assert not np.array_equal(_bits(tr.params.to_host()), _bits(p))
    finally:
        tr.close()
        if tr2 is not None:
            tr2.close()


# ---- 4. errors before any launch ---------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(ctx, monkeypatch):
    C = 5
    weights, x, cues, tags = _step_case("DSRG")
    tr = secdsrg.SegTrainer("DSRG", weights, C, precision=_lib.PREC_F32, ctx=ctx)
    other = cam = None
    try:
        sg = tr.net._grad
        n = sg.grad_elems
        canary = np.full((n + GUARD,), CANARY, np.float32)
        x48 = ref.net_input(1, 64, 48, 5)
        with tr.net.forward_dev(x48) as prob:
            before = _bits(prob.to_host())
        other = _lib.Context(0)
        sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
        cam = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, sd, 20, _lib.PREC_F16)
        with DeviceMaps.from_host(ctx, canary) as p, DeviceMaps.from_host(ctx, canary) as g, DeviceMaps.from_host(ctx, canary) as a, \
                DeviceMaps.from_host(ctx, canary) as m:
            calls = [lambda: sg.sgd_accumulate(p.ptr, g.ptr, a.ptr, 5e-4, 1, elems=n - 1),
                     lambda: sg.sgd_accumulate(p.ptr, g.ptr, a.ptr, 5e-4, 1, ctx=other),
                     lambda: sg.sgd_accumulate(p.ptr, None, a.ptr, 5e-4, 1),
                     lambda: sg.sgd_apply(p.ptr, a.ptr, m.ptr, 1e-4, 0.9, elems=n + 4),
                     lambda: sg.sgd_apply(p.ptr, a.ptr, m.ptr, 1e-4, 0.9, ctx=other),
                     lambda: sg.sgd_apply(p.ptr, a.ptr, None, 1e-4, 0.9),
                     lambda: sg.load_params(p.ptr, elems=n - 1),
                     lambda: sg.load_params(p.ptr, ctx=other),
                     lambda: sg.load_params(p.ptr, net=cam)]
            for i, call in enumerate(calls):
                with pytest.raises(_lib.WscError) as ei:
                    call()
                assert ei.value.status == _lib.WSC_ERR_INVALID, i
            for d in (p, g, a, m):
                assert np.array_equal(_bits(d.to_host()), _bits(canary))  # nothing was launched
        with tr.net.forward_dev(x48) as prob:
            assert np.array_equal(_bits(prob.to_host()), before)  # ... on the net either
        with pytest.raises(ValueError):
            tr.net.load_params_dev(np.zeros((n - 1,), np.float32))

        # a mis-shaped cues array: step raises and hands back every buffer it took
        handed = []
        alloc0 = ctx.alloc

        def alloc(nbytes, pooled=False):
            handed.append(alloc0(nbytes, pooled=pooled))
            return handed[-1]

        monkeypatch.setattr(ctx, "alloc", alloc)
        with pytest.raises(ValueError):
            tr.step(x, cues[:, :8], tags, MEAN, CRF_CFG)
        monkeypatch.undo()
        assert handed and not [b for b in handed if b.ptr is not None]
        assert tr.calls == 0 and np.array_equal(_bits(tr.params.to_host()), _bits(sgd.flatten(*sgd.layout_of("DSRG", weights), weights)))
    finally:
        tr.close()
        if cam is not None:
            cam.close()
        if other is not None:
            other.close()
