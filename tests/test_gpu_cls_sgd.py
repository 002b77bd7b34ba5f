"""GPU: the update half of a 01_train step (csrc/sgd.hip, csrc/repack.hip; wsc_cls_param_layout, wsc_cls_sgd_step, wsc_net_cls_load_params;
vgg16_cam.CAM.load_params_dev, cls_train.ClsTrainer) against tests/cls_sgd_ref.py.

  step bits    parameters and momentum bit for bit those of the float32 one-rounding-per-operation restatement (the definition), in
               the 16-byte and in the scalar form, Nesterov on and off, over three steps from a zero momentum; the gradient and the
               canaries untouched; a NaN gradient stays in its element.
  repack       after load_params_dev a model has the bits of a model created from the same floats and running statistics: the
               features, the whole tape, the gradient of the backward pass, and forward_batch's CAM and score -- the last two are
               the test of the BatchNorm fold on the device (double division and square root against the host's).
  trainer      ClsTrainer.step = cls_train.grad_step on a fresh model from the previous host parameters, the restatement on the
               host: metrics, parameters, momentum and running statistics to the bit; save / load resumes to the bit.
  refusals     every WSC_ERR_INVALID of the two entries, with nothing written."""
import numpy as np
import pytest

from oracle import cnn_ref
from tests import cls_grad_ref as gref
from tests import cls_sgd_ref as ref
from tests.test_gpu_cls_grad import CANARY, GUARD, _bits, _guarded
from wsscam import _lib, cls_train
from wsscam.net import m7_cam, vgg16_cam
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

PRECS = {"f16x3": _lib.PREC_F16X3, "f32": _lib.PREC_F32, "f16": _lib.PREC_F16}
C = 20
HW = (33, 33)
# (root, BatchNorm, pools): VGG16 with and without BatchNorm on torch's pools, M7 on a Keras session's
NETS = {"vgg16-bn": ("vgg16", True, None), "vgg16-nobn": ("vgg16", False, None), "m7-keras": ("m7", True, gref.KERAS_POOLS)}


def _np_sd(sd):
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}


def fresh_model(net, sd, precision, ctx=None):
    """a model of its own (the tests below rewrite its net), on `ctx` where given"""
    root, bn, pools = NETS[net]
    cls = vgg16_cam.CAM if root == "vgg16" else m7_cam.CAM
    m = cls(None, "voc12", "", C, None, precision=precision, pooling=None if pools is None else list(pools))
    m._ctx = ctx
    m.load_state_dict(sd)
    m.eval().cuda(0)
    return m


def base_sd(net):
    """the real-width weights of tests/cls_grad_ref.py; an M7 dict carries its Grad-CAM head, which is no parameter"""
    root, bn, pools = NETS[net]
    sd = _np_sd(gref.state_dict(root, bn))
    if root == "m7":
        rng = np.random.default_rng(77)
        sd["gradcam_weights"] = (0.05 * rng.standard_normal((256, C))).astype(np.float32)
    return sd


# ---- 1. step bits ---------------------------------------------------------------------------------------------------------------------
def _step_data(n):
    rng = np.random.default_rng(n % 1000 + 5)
    p = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)
    g = (rng.standard_normal(n) * 2.0 ** rng.integers(-10, 11, n)).astype(np.float32)
    p[0:8] = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e-39, 0.0, -0.0]  # signed zeros, float32 denormals
    g[0:8] = [0.0, -0.0, 0.0, 1e-41, -1.4e-45, 1e-44, -0.0, 1.0]    # -0.0, denormals; lr g underflows at [3:6]
    p[8:12] = [1.0, -2.5e38, 0.0, 3.0e38]
    g[8:12] = [3.0e38, -3.0e38, 2.9e38, -1.5e38]                     # near the top of the range: lr g is still finite
    g[100:164] = 0.0                                                # a zero gradient: the momentum alone
    return p, g


@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "plain"])
@pytest.mark.parametrize("form", ["aligned", "offset"])
def test_step_bits(form, nesterov):
    from tests.test_gpu_cls_grad import model

    m = model("m7", True, None, "f32")
    ctx, grad = m.ctx, m.cls_grad()
    sd = _np_sd(gref.state_dict("m7", True))
    ent, n, grad_elems = ref.layout(sd, "m7", C)
    # the layout: the gradient layout unchanged in front, the Linear as torch's [C][F] and its bias behind it, no gaps
    assert grad.param_elems == n and grad.grad_elems == grad_elems and grad.param_layout[:len(grad.layout)] == [dict(e, linear=False) for e in grad.layout]
    assert [(e["name"], e["offset"]) for e in grad.param_layout] == [(e[0], e[1]) for e in ent]
    assert grad.param_layout[-2]["shape"] == (C, 256) and grad.param_layout[-2]["linear"] and grad.param_layout[-1]["shape"] == (C,)
    assert grad_elems % 64 == 0  # the tail is on the 16-byte grid: what wsc_cls_loss asks of w_dev / grad_w_dev
    p0, g0 = _step_data(n)
    lead = 0 if form == "aligned" else 1  # offset: the buffers start one float into their allocation -> the scalar form
    can = np.full((lead,), CANARY, np.float32)
    mo = 0.9
    with _guarded(ctx, np.concatenate([can, p0])) as pd, _guarded(ctx, np.concatenate([can, g0])) as gd, \
            _guarded(ctx, np.concatenate([can, np.zeros(n, np.float32)])) as md:
        assert pd.ptr % 16 == 0 and gd.ptr % 16 == 0 and md.ptr % 16 == 0
        p, mom = p0, np.zeros(n, np.float32)

        def check(k, want_p, want_m, want_g):
            for name, buf, want in (("param", pd, want_p), ("momentum", md, want_m), ("gradient", gd, want_g)):
                got = buf.to_host()
                assert np.array_equal(_bits(got[:lead]), _bits(can)) and np.array_equal(_bits(got[lead + n:]), _bits(np.full(GUARD, CANARY, np.float32))), \
                    (name, k, "a store outside the buffer")
                diff = _bits(got[lead:lead + n]) != _bits(want)
                assert not diff.any(), (name, k, int(diff.sum()), np.flatnonzero(diff)[:8])

        for k, lr in enumerate((0.01, 0.005, 0.02)):
            grad.sgd_step(pd.ptr + 4 * lead, gd.ptr + 4 * lead, md.ptr + 4 * lead, lr, mo, nesterov)
            p, mom = ref.sgd_step32(p, g0, mom, lr, mo, nesterov)
            check(k, p, mom, g0)
        # ([3]: lr g is a denormal; [4], [5]: it underflows to zero and the element stands still)
        assert np.isfinite(p).all() and p[3] != p0[3] and mom[3] != 0 and (mom[4:6] == 0).all() and (p[4:6] == p0[4:6]).all() and mom[7] != 0
        # a NaN gradient: NaN in p and m at that element and nowhere else
        g1 = g0.copy()
        g1[13] = np.nan
        _lib.check(ctx._lib.wsc_memcpy_h2d(ctx.h, gd.ptr + 4 * lead, g1.ctypes.data, g1.nbytes))
        ctx.sync()
        grad.sgd_step(pd.ptr + 4 * lead, gd.ptr + 4 * lead, md.ptr + 4 * lead, 0.01, mo, nesterov)
        p, mom = ref.sgd_step32(p, g1, mom, 0.01, mo, nesterov)
        assert np.isnan(p[13]) and np.isnan(mom[13]) and np.isfinite(np.delete(p, 13)).all() and np.isfinite(np.delete(mom, 13)).all()
        got_p, got_m = pd.to_host()[lead:lead + n], md.to_host()[lead:lead + n]
        assert np.isnan(got_p[13]) and np.isnan(got_m[13])
        keep = np.arange(n) != 13
        assert np.array_equal(_bits(got_p[keep]), _bits(p[keep])) and np.array_equal(_bits(got_m[keep]), _bits(mom[keep]))
        assert np.array_equal(_bits(gd.to_host()[lead:lead + n][keep]), _bits(g1[keep]))


# ---- 2. repack equals creation --------------------------------------------------------------------------------------------------------
def _edge_channels(w, rng):
    """the packing's edge cases in output channels 0 .. 5 of a weight [Cout][...]"""
    w = w.copy()
    flat = w.reshape(w.shape[0], -1)
    k = flat.shape[1]
    flat[0] = 0.0                                               # an output channel of zeros
    flat[1] = (1e-40 * rng.uniform(-1, 1, k)).astype(np.float32)
    flat[1, 3] = 1e-40                                          # one whose maximum is 1e-40
    flat[2] = np.clip(flat[2], -0.1, 0.1)
    flat[2, 5] = 0.125                                          # one whose maximum is a power of two
    flat[3] = np.clip(flat[3], -0.1, 0.1)
    flat[3, 7] = np.nextafter(np.float32(0.25), np.float32(0))  # one just below a power of two
    flat[4] = -np.abs(flat[4])
    flat[4, k - 1] = -3.0                                       # one whose maximum is negative
    flat[5] = (flat[5] * 2.0 ** rng.integers(-20, 1, k)).astype(np.float32)  # one spread over 2^20
    return w


def edge_case_sd(sd0, root):
    """sd0 with every trainable tensor changed (the convention of test_gpu_irn_sgd.edge_case_sd), the packing's edge cases in the
    first conv (the small form), a middle one, the last one and the classifier (VGG16's CAM head), and one gamma of 0"""
    rng = np.random.default_rng(31)
    sd1 = dict(sd0)
    names = gref.param_names(root, sd0) + [root + ".classifier.0.weight", root + ".classifier.0.bias"]
    for k in names:
        v = sd0[k]
        sd1[k] = (v * (1 + 0.25 * rng.standard_normal(v.shape)) + 0.01 * rng.standard_normal(v.shape)).astype(np.float32)
    convs = [n for n in names if n.endswith(".weight") and sd0[n].ndim == 4]
    for name in (convs[0], convs[len(convs) // 2], convs[-1], root + ".classifier.0.weight"):
        sd1[name] = _edge_channels(sd1[name], rng)
    gammas = [n for n in names if n.endswith(".weight") and sd0[n].ndim == 1]
    if gammas:
        sd1[gammas[1]][9] = 0.0
    return sd1


def _all_bits(m, xb):
    """the features, every tape entry, the gradient buffer and forward_batch's CAM and score of one model, as uint32; the running
    statistics stay (bn_keep=None)"""
    out = {}
    feat, tape = m.forward_train_dev(gref.net_input(HW), keep=True, bn_keep=None)
    with feat, tape:
        out["feat"] = _bits(feat.to_host())
        for e in tape.entries:
            out["tape:" + e["name"]] = _bits(tape.entry(e["name"]))
        dfeat = (1e-3 * np.random.default_rng(HW[0]).standard_normal(feat.shape)).astype(np.float32)
        with DeviceMaps.from_host(m.ctx, dfeat) as dd, m.backward_dev(tape, dd) as g:
            out["gradient"] = _bits(g.maps.to_host())
    cam, score = m.forward_batch(xb, want_score=True)
    out["cam"], out["score"] = _bits(cam), _bits(score)
    return out


@pytest.mark.parametrize("prec", list(PRECS), ids=list(PRECS))
@pytest.mark.parametrize("net", list(NETS), ids=list(NETS))
def test_repack_equals_creation(net, prec):
    root, bn, pools = NETS[net]
    sd0 = base_sd(net)
    a = fresh_model(net, sd0, PRECS[prec])
    ctx = a.ctx
    b = None
    try:
        xb = np.random.default_rng(17).normal(0, 1, (2, 2, 3, HW[0], HW[1])).astype(np.float32)
        grad = a.cls_grad()
        flat0 = grad.flat_params(sd0)
        assert np.array_equal(_bits(flat0), _bits(ref.flat_params(sd0, root, C)))
        before = _all_bits(a, xb)
        a.load_params_dev(flat0)  # its own parameters and running statistics: nothing changes, the inference fold included
        again = _all_bits(a, xb)
        for k in before:
            assert np.array_equal(before[k], again[k]), ("reload", k, int((before[k] != again[k]).sum()), before[k].size)
        sd1 = edge_case_sd(sd0, root)
        if bn:  # one forward pass moves the running statistics; one variance of 0 on top
            a.forward_train_dev(gref.net_input(HW), keep=False).free()
            run = a.bn_running()
            moved = [k for k in run if not np.array_equal(run[k], sd0[k])]
            assert len(moved) == len(run)
            key = a.bn_keys()[2] + ".running_var"
            run[key][4] = 0.0
            flat_run = np.concatenate([run[k + "." + s] for k in a.bn_keys() for s in ("running_mean", "running_var")])
            _lib.check(ctx._lib.wsc_memcpy_h2d(ctx.h, a.bn_running_dev().ptr, flat_run.ctypes.data, flat_run.nbytes))
            ctx.sync()
            sd1.update(run)
        with DeviceMaps.from_host(ctx, grad.flat_params(sd1)) as fd:  # a DeviceMaps is read in place
            a.load_params_dev(fd)
        b = fresh_model(net, sd1, PRECS[prec], ctx=ctx)
        got, want = _all_bits(a, xb), _all_bits(b, xb)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()), got[k].size)
        assert ctx.range_status() == 0
        for k in ("feat", "gradient", "cam", "score"):  # the weights did change
            assert got[k].any() and not np.array_equal(got[k], before[k]), k
    finally:
        a._release_net()
        if b is not None:
            b._release_net()
        ctx.close()


# ---- 3. the trainer is the composition --------------------------------------------------------------------------------------------------
POOL = {"vgg16": "mean", "m7": "max"}


def _trainer_case():
    rng = np.random.default_rng(9)
    return gref.net_input(HW), (rng.random((gref.B, C)) < 0.3).astype(np.float32), np.array([1.0, 2.0], np.float32)


@pytest.mark.parametrize("net", ["m7-keras", "vgg16-bn"])
def test_trainer_is_the_composition(ctx, net, monkeypatch, tmp_path):
    root, bn, pools = NETS[net]
    sd0 = base_sd(net)
    x, targets, sw = _trainer_case()
    prec = _lib.PREC_F16X3
    m = fresh_model(net, sd0, prec, ctx=ctx)
    m2 = m3 = tr2 = tr3 = f = None
    tr = cls_train.ClsTrainer(m, POOL[root], C)
    try:
        p, mom = ref.flat_params(sd0, root, C), np.zeros(ref.layout(sd0, root, C)[1], np.float32)
        assert np.array_equal(_bits(tr.params.to_host()), _bits(p)) and not tr.mom.to_host().any()
        sd_prev, record = sd0, []
        loss = cls_train.ClsLoss(ctx, POOL[root], C)
        for k, lr in enumerate((0.01, 0.004)):
            assert tr.global_step == k
            downloads, handed, to_host0, alloc0 = [], [], ctx.to_host, ctx.alloc

            def to_host(buf, shape, dtype, offset_bytes=0):
                downloads.append((tuple(shape), np.dtype(dtype)))
                return to_host0(buf, shape, dtype, offset_bytes=offset_bytes)

            def alloc(nbytes, pooled=False):
                handed.append(alloc0(nbytes, pooled=pooled))
                return handed[-1]

            monkeypatch.setattr(ctx, "to_host", to_host)
            monkeypatch.setattr(ctx, "alloc", alloc)
            got = tr.step(x, targets, lr, sw)
            monkeypatch.undo()
            assert downloads == [((6,), np.dtype(np.float64))]  # the six loss values and nothing else
            assert handed and [h.ptr for h in handed if h.ptr is not None] == []  # a step frees what it allocates
            # the long way round: a fresh model from the previous host parameters, grad_step, the restatement on the host
            fm = fresh_model(net, sd_prev, prec, ctx=ctx)
            try:
                want, head, grads = cls_train.grad_step(fm, loss, x, targets, sw)
                with head.feat, head.w, head.bias, grads:
                    g = np.concatenate([grads.maps.to_host(), head.w.to_host().ravel(), head.bias.to_host()])
                run = fm.bn_running()
            finally:
                fm._release_net()
            assert got == want, k  # step k computes with the parameters step k - 1 left in the net, to the bits
            p, mom = ref.sgd_step32(p, g, mom, lr, 0.9, True)
            hp, hm = tr.params_host(), tr.momentum_host()
            # (the reference's layout tells a BatchNorm net by its running statistics: the rest of the dict comes along)
            dp_ = _bits(ref.flat_params(dict(sd_prev, **hp), root, C)) != _bits(p)
            dm_ = _bits(ref.flat_params(dict(sd_prev, **hm), root, C)) != _bits(mom)
            assert set(hp) == set(hm) == {e[0] for e in ref.layout(sd_prev, root, C)[0]}
            assert not dp_.any() and not dm_.any(), (k, int(dp_.sum()), int(dm_.sum()))
            assert np.isfinite(p).all() and np.abs(g).max() > 0 and np.abs(g[-C:]).max() > 0
            got_run = m.bn_running()
            assert set(got_run) == set(run) and all(np.array_equal(_bits(got_run[n]), _bits(run[n])) for n in run)
            assert all(not np.array_equal(run[n], sd_prev[n]) for n in run)  # the running statistics moved
            sd_prev = dict(sd_prev)
            sd_prev.update(hp)
            sd_prev.update(run)
            record.append((got, p.copy(), mom.copy()))
            print("trainer %s step %d: loss %.6f, lr %g, max |p - p0| %.3e" % (net, k, got["loss"], lr, np.abs(p - ref.flat_params(sd0, root, C)).max()))
        assert hp[root + ".layer1.0.weight"].shape == (64, 3, 3, 3) and hp[root + ".classifier.0.weight"].shape == (C, sd0[root + ".classifier.0.weight"].shape[1])
        # state_dict(): the full dict, the wrapper's own copy refreshed, and a fresh model from it is the trained one
        sd_t = tr.state_dict()
        assert set(sd_t) == set(sd0) and all(np.array_equal(_bits(sd_t[n]), _bits(sd_prev[n])) for n in sd_prev)
        assert all(np.array_equal(m._sd[n], sd_t[n]) for n in sd_t)
        xb = np.random.default_rng(19).normal(0, 1, (2, 2, 3, HW[0], HW[1])).astype(np.float32)
        f = fresh_model(net, sd_t, prec, ctx=ctx)
        got_b, want_b = _all_bits(m, xb), _all_bits(f, xb)
        for n in want_b:
            assert np.array_equal(got_b[n], want_b[n]), ("state_dict", n, int((got_b[n] != want_b[n]).sum()))
        # save after step 1 -> load -> step 2 = the uninterrupted run
        m2 = fresh_model(net, sd0, prec, ctx=ctx)
        # (both through fit: lr_of_step sees the trainer's step count, the means are those of the one batch)
        with cls_train.ClsTrainer(m2, POOL[root], C) as tr2:
            ep = cls_train.fit(tr2, [(x, targets, sw)], lambda k: {0: 0.01}[k])
            assert len(ep) == 1 and all(ep[0][n] == record[0][0][n] for n in ("loss", "binary_accuracy", "f1")) and ep[0]["samples"] == gref.B
            path = str(tmp_path / "cls_trainer.npy")
            tr2.save(path)
        m2._release_net()
        m3 = (vgg16_cam.CAM if root == "vgg16" else m7_cam.CAM)(None, "voc12", "", C, None, precision=prec, pooling=None if pools is None else list(pools))
        m3._ctx = ctx
        tr3 = cls_train.ClsTrainer.load(path, m3, POOL[root], C)
        assert tr3.global_step == 1
        ep = cls_train.fit(tr3, [(x, targets, sw)], lambda k: {1: 0.004}[k], steps_per_epoch=1)
        assert len(ep) == 1 and all(ep[0][n] == record[1][0][n] for n in ("loss", "binary_accuracy", "f1")) and tr3.global_step == 2
        assert np.array_equal(_bits(tr3.params.to_host()), _bits(record[1][1])) and np.array_equal(_bits(tr3.mom.to_host()), _bits(record[1][2]))
    finally:
        for t in (tr, tr3):
            if t is not None:
                t.close()
        for mm in (m, m2, m3, f):
            if mm is not None:
                mm._release_net()


def test_trainer_failures_leave_everything_as_it_was(ctx, monkeypatch):
    """an exception mid-step leaks nothing; a NaN input is a FloatingPointError before the update: parameters, momentum and the
    packed weights keep their bits (the running statistics have moved, as the docstring says)"""
    net = "m7-keras"
    x, targets, sw = _trainer_case()
    m = fresh_model(net, base_sd(net), _lib.PREC_F16X3, ctx=ctx)
    try:
        with cls_train.ClsTrainer(m, "max", C) as tr:
            tr.step(x, targets, 0.01, sw)
            xb = np.random.default_rng(19).normal(0, 1, (2, 2, 3, HW[0], HW[1])).astype(np.float32)
            p0, m0, packed0 = tr.params.to_host(), tr.mom.to_host(), _all_bits(m, xb)
            handed, alloc0 = [], ctx.alloc

            def alloc(nbytes, pooled=False):
                handed.append(alloc0(nbytes, pooled=pooled))
                return handed[-1]

            def boom(*a, **k):
                raise RuntimeError("mid-step")

            monkeypatch.setattr(ctx, "alloc", alloc)
            monkeypatch.setattr(tr.grad, "sgd_step", boom)
            with pytest.raises(RuntimeError, match="mid-step"):
                tr.step(x, targets, 0.01, sw)
            monkeypatch.undo()
            assert handed and [h.ptr for h in handed if h.ptr is not None] == [] and tr.global_step == 1
            bad = x.copy()
            bad[1, 2, 17, 5] = np.nan
            monkeypatch.setattr(ctx, "alloc", alloc)
            del handed[:]
            try:
                with pytest.raises(FloatingPointError):
                    tr.step(bad, targets, 0.01, sw)
            finally:
                monkeypatch.undo()
                ctx.range_status(clear=True)
            assert handed and [h.ptr for h in handed if h.ptr is not None] == [] and tr.global_step == 1
            assert np.array_equal(_bits(tr.params.to_host()), _bits(p0)) and np.array_equal(_bits(tr.mom.to_host()), _bits(m0))
            packed1 = _all_bits(m, xb)
            assert all(np.array_equal(packed0[k], packed1[k]) for k in packed0)
            with pytest.raises(ValueError):
                tr.step(x, targets, float("nan"), sw)
        with pytest.raises(ValueError):
            tr.step(x, targets, 0.01, sw)  # closed
    finally:
        ctx.range_status(clear=True)
        m._release_net()


# ---- 4. refusals before any launch ----------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(ctx):
    sd = base_sd("vgg16-bn")
    m = fresh_model("vgg16-bn", sd, _lib.PREC_F16X3)
    other = fresh_model("m7-keras", base_sd("m7-keras"), _lib.PREC_F16X3)
    mctx, net, grad = m.ctx, m._ensure_net(), m.cls_grad()
    n = grad.param_elems
    canary = np.full((n,), CANARY, np.float32)
    gc_net = cam = gc_grad = None
    try:
        xb = np.random.default_rng(17).normal(0, 1, (2, 2, 3, HW[0], HW[1])).astype(np.float32)
        before = _all_bits(m, xb)
        run = m.bn_running_dev()
        run0 = run.to_host()
        with DeviceMaps.from_host(mctx, canary) as p, DeviceMaps.from_host(mctx, canary) as g, DeviceMaps.from_host(mctx, canary) as mo:

            def invalid(fn, text=None):
                with pytest.raises(_lib.WscError) as ei:
                    fn()
                assert ei.value.status == _lib.WSC_ERR_INVALID and (text is None or text in str(ei.value)), str(ei.value)

            invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, 0.01, elems=n - 1))
            invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, 0.01, elems=grad.grad_elems))  # the gradient layout is not the training layout
            invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, 0.01, ctx=ctx))  # a foreign context
            invalid(lambda: grad.sgd_step(None, g.ptr, mo.ptr, 0.01))
            invalid(lambda: grad.sgd_step(p.ptr, None, mo.ptr, 0.01))
            invalid(lambda: grad.sgd_step(p.ptr, g.ptr, None, 0.01))
            for lr in (float("nan"), float("inf"), -1e-3):
                invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, lr), "lr")
            for mu in (float("nan"), -0.1, 1.0, 1.5):
                invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, 0.01, momentum=mu), "momentum")
            for nest in (2, -1):
                invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, 0.01, nesterov=nest), "nesterov")
            invalid(lambda: grad.load_params(p.ptr, run.ptr, elems=n + 1))
            invalid(lambda: grad.load_params(p.ptr, run.ptr, elems=grad.grad_elems))
            invalid(lambda: grad.load_params(p.ptr, run.ptr, ctx=ctx))
            invalid(lambda: grad.load_params(None, run.ptr))
            invalid(lambda: grad.load_params(p.ptr, run.ptr, net=other._ensure_net()))  # a wsc_cls_grad of another net
            invalid(lambda: other.cls_grad().load_params(p.ptr, None, elems=other.cls_grad().param_elems, net=net))
            cam_sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
            cam = _lib.Net(mctx, _lib.ARCH_RESNET50_CAM, cam_sd, 20, _lib.PREC_F16)
            invalid(lambda: grad.load_params(p.ptr, run.ptr, net=cam))  # a net of another arch
            # a VGG16 net built with gradcam_weights: its head is not the classifier
            gsd = dict(m._sd)
            gsd["gradcam_weights"] = (0.05 * np.random.default_rng(3).standard_normal((1024, C))).astype(np.float32)
            gc_net = _lib.Net(mctx, _lib.ARCH_VGG16_CAM, gsd, C, _lib.PREC_F16X3)
            gc_grad = _lib.ClsGrad(gc_net, gsd)
            assert gc_grad.param_elems == n
            invalid(lambda: gc_grad.load_params(p.ptr, None), "gradcam_weights")
            mctx.sync()
            for buf in (p, g, mo):  # nothing was launched
                assert np.array_equal(_bits(buf.to_host()), _bits(canary))
        assert np.array_equal(_bits(run.to_host()), _bits(run0))
        after = _all_bits(m, xb)
        assert all(np.array_equal(before[k], after[k]) for k in before)  # the net was not written
        # the Python layer
        with pytest.raises(ValueError):
            m.load_params_dev(np.zeros(n - 1, np.float32))
        with DeviceMaps.from_host(ctx, canary[:16]) as foreign, pytest.raises(ValueError):
            m.load_params_dev(foreign)
        with pytest.raises(ValueError):
            cls_train.ClsTrainer(m, "mean", C, ctx=ctx)  # a trainer whose model lives on another context
        with pytest.raises(ValueError):
            cls_train.ClsTrainer(m, "mean", C, momentum=1.0)
        with pytest.raises(ValueError):
            cls_train.ClsTrainer(m, "mean", 5)  # another class count than the net's
        with pytest.raises(ValueError):
            grad.flat_params({k: v for k, v in sd.items() if k != "vgg16.layer3.3.bias"})
    finally:
        for o in (gc_grad, gc_net, cam):
            if o is not None:
                o.close()
        mc, oc = m.ctx, other.ctx
        m._release_net()
        other._release_net()
        mc.close()
        oc.close()
