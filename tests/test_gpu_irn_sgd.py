"""GPU: the update half of an IRNet training step and the closing dp_mean pass (csrc/sgd.hip, csrc/repack.hip, csrc/irn_grad.hip; wsc_irn_sgd_step,
wsc_net_irn_load_params, wsc_channel_mean_nchw, wsc_net_set_mean_shift; misc.torchutils.PolyOptimizer, irn_train.IrnTrainer)
against tests/irn_sgd_ref.py.

  step bits    parameters and momentum bit for bit those of the float32 non-fused restatement (the definition), in the 16-byte
               and in the scalar form, over three steps from a zero momentum; the gradient and the canaries untouched.
  repack       after load_params_dev a model has the bits of a model created from the same floats: head outputs, the whole tape,
               the gradient of the backward pass, the inference outputs.
  trainer      IrnTrainer.step = a fresh model from the previous host parameters, AffinityLoss.grad_step, the restatement on the
               host: losses, parameters and momentum to the bit.
  dp_mean      the double per-channel mean within 1e-12 max|x| of numpy's float64 mean (another summation order: not to the bit
               against numpy, to the bit against itself); fit_dp_mean = the oracle on the downloaded dp_out, rounded once."""
import numpy as np
import pytest

from oracle import cnn_ref, irn_ref
from tests import irn_loss_ref
from tests import irn_sgd_ref as ref
from tests.test_gpu_irn_grad import CANARY, GUARD, _bits, _canary, _checked, _guarded, model, net_input
from wsscam import _lib, irn_train
from wsscam.misc.indexing import PathIndex
from wsscam.misc.torchutils import PolyOptimizer
from wsscam.net import m7_irn, resnet50_irn, vgg16_irn
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

PRECS = {"f16x3": _lib.PREC_F16X3, "f32": _lib.PREC_F32, "f16": _lib.PREC_F16, "bf16x3": _lib.PREC_BF16X3}


def _np_sd(sd):
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}


def fresh_model(arch, sd, ctx=None, precision=None):
    """a model of its own (the tests below rewrite its net), on `ctx` where given"""
    if arch == "resnet50":
        m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=64, stride=4, precision=precision)
    elif arch == "vgg16":
        m = vgg16_irn.EdgeDisplacement(None, "voc12", "", 20, None, crop_size=64, stride=4, precision=precision or _lib.PREC_F16X3)
    else:
        m = m7_irn.EdgeDisplacement(None, "voc12", "", 20, None, crop_size=64, stride=4, precision=precision)
    m._ctx = ctx
    m.load_state_dict(sd)
    m.eval().cuda(0)
    return m


def base_sd(arch):
    if arch == "resnet50":
        return _np_sd(irn_ref.make_resnet50_irn_state_dict(seed=3))
    if arch == "vgg16":
        return _np_sd(irn_ref.make_vgg16_irn_state_dict(seed=2))
    return _np_sd(irn_ref.make_m7_irn_state_dict(seed=4))


# ---- 1. step bits ---------------------------------------------------------------------------------------------------------------------
def _step_data(n, b):
    rng = np.random.default_rng(n % 1000 + 5)
    p = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)
    g = (rng.standard_normal(n) * 2.0 ** rng.integers(-10, 11, n)).astype(np.float32)
    p[0:8] = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e-39, 0.0, -0.0]  # signed zeros, float32 denormals
    g[0:8] = [0.0, 0.0, 0.0, 1e-41, -1.4e-45, 0.0, -0.0, 1.0]
    g[100:164] = 0.0  # a zero gradient: weight decay and momentum alone
    for i in (b - 1, b, b + 1):  # the group boundary and its neighbours: O(1) values, so that a wrong rate changes the bits
        p[i], g[i] = 0.75 + 0.01 * (i - b), -1.25
    return p, g


@pytest.mark.parametrize("form", ["aligned", "offset"])
@pytest.mark.parametrize("arch", ["resnet50", "vgg16", "m7"])
def test_step_bits(arch, form):
    m, sd = model(arch)
    ctx, grad = m.ctx, m.irn_grad()
    n, b = grad.grad_elems, ref.boundary(sd, arch)
    assert n == ref.layout(sd, arch)[1] and [e["name"] for e in grad.layout] == [e[0] for e in ref.layout(sd, arch)[0]]
    assert [e["offset"] for e in grad.layout] == [e[1] for e in ref.layout(sd, arch)[0]] and b % 2 == 1  # (the one-float bias)
    p0, g0 = _step_data(n, b)
    lead = 0 if form == "aligned" else 1  # offset: the buffers start one float into their allocation -> the scalar form
    can = np.full((lead,), CANARY, np.float32)
    wd, mo = 1e-4, 0.9
    with _guarded(ctx, np.concatenate([can, p0])) as pd, _guarded(ctx, np.concatenate([can, g0])) as gd, \
            _guarded(ctx, np.concatenate([can, np.zeros(n, np.float32)])) as md:
        assert pd.ptr % 16 == 0 and gd.ptr % 16 == 0 and md.ptr % 16 == 0
        p, mom = p0, np.zeros(n, np.float32)
        for k in range(3):
            lr_e, lr_d = ref.poly_lrs(0.1, 4, 0.9, k)
            grad.sgd_step(pd.ptr + 4 * lead, gd.ptr + 4 * lead, md.ptr + 4 * lead, lr_e, lr_d, wd, mo)
            p_prev = p
            p, mom = ref.sgd_step32(p, g0, mom, b, lr_e, lr_d, wd, mo)
            got_p, got_m, got_g = pd.to_host(), md.to_host(), gd.to_host()
            for name, got, want in (("param", got_p, p), ("momentum", got_m, mom), ("gradient", got_g, g0)):
                assert np.array_equal(_bits(got[:lead]), _bits(can)) and np.array_equal(_bits(got[lead + n:]), _bits(np.full(GUARD, CANARY, np.float32))), \
                    (name, k, "a store outside the buffer")
                diff = _bits(got[lead:lead + n]) != _bits(want)
                assert not diff.any(), (name, k, int(diff.sum()), np.flatnonzero(diff)[:8])
            # the boundary: b - 1 took the edge rate, b and b + 1 the dp rate -- and the other rate gives other bits
            for i, lr, other in ((b - 1, lr_e, lr_d), (b, lr_d, lr_e), (b + 1, lr_d, lr_e)):
                assert got_p[lead + i] == np.float32(p_prev[i] - np.float32(lr) * mom[i])
                assert got_p[lead + i] != np.float32(p_prev[i] - np.float32(other) * mom[i])
        assert np.isfinite(p).all() and (p[2:6] != p0[2:6]).any()


# ---- 2. repack equals creation --------------------------------------------------------------------------------------------------------
def edge_case_sd(sd0, arch):
    """sd0 with every head tensor changed, and the packing's edge cases in the output channels of six layers"""
    rng = np.random.default_rng(31)
    sd1 = dict(sd0)
    for k, v in sd0.items():
        if k.startswith("fc_"):
            sd1[k] = (v * (1 + 0.25 * rng.standard_normal(v.shape)) + 0.01 * rng.standard_normal(v.shape)).astype(np.float32)
    t = {"resnet50": ("fc_edge6", "fc_dp7.3", "fc_dp6", "fc_dp7"), "vgg16": ("fc_edge6", "fc_dp7.3", "fc_dp6", "fc_dp7"),
         "m7": ("fc_edge4", "fc_dp5.3", "fc_dp4", "fc_dp5")}[arch]
    for name in ("fc_edge1.0.weight", "fc_dp2.0.weight", t[2] + ".0.weight", t[3] + ".0.weight"):  # (the last two have a w_rot)
        w = sd1[name].copy()
        cin = w.shape[1]
        w[0] = 0.0                                              # an output channel of zeros
        w[1] = (1e-40 * rng.uniform(-1, 1, w[1].shape)).astype(np.float32)
        w[1, 3] = 1e-40                                         # one whose maximum is 1e-40
        w[2] = np.clip(w[2], -0.1, 0.1)
        w[2, 5] = 0.125                                         # one whose maximum is a power of two
        w[3] = np.clip(w[3], -0.1, 0.1)
        w[3, 7] = np.nextafter(np.float32(0.25), np.float32(0))  # one just below a power of two
        w[4] = -np.abs(w[4])
        w[4, cin - 1] = -3.0                                    # one whose maximum is negative
        w[5] = (w[5] * 2.0 ** rng.integers(-20, 1, w[5].shape)).astype(np.float32)  # one spread over 2^20
        sd1[name] = w
    w6 = -np.abs(sd1[t[0] + ".weight"])
    w6[0, 11] = -0.125
    sd1[t[0] + ".weight"] = np.minimum(w6, 0).clip(-0.125, 0).astype(np.float32)  # one column: a negative maximum, a power of two
    w7 = sd1[t[1] + ".weight"].copy()
    w7[0] = np.clip(w7[0], -0.2, 0.2)
    w7[0, 9] = np.nextafter(np.float32(0.25), np.float32(0))    # two columns: just below a power of two,
    w7[1] = (w7[1] * 2.0 ** rng.integers(-20, 1, w7[1].shape)).astype(np.float32)  # and spread over 2^20
    sd1[t[1] + ".weight"] = w7
    return sd1


def _all_bits(m, N, S, xb):
    """edge_out, dp_out, every tape entry, the gradient buffer and the inference outputs of one model, as uint32"""
    out = {}
    x = net_input(N, S)
    edge, dp, tape = m.forward_train_dev(x, keep=True)
    with edge, dp, tape:
        out["edge_out"], out["dp_out"] = _bits(edge.to_host()), _bits(dp.to_host())
        for e in tape.entries:
            out["tape:" + e["name"]] = _bits(tape.entry(e["name"]))
        rng = np.random.default_rng(S + N)
        with DeviceMaps.from_host(m.ctx, (1e-3 * rng.standard_normal(edge.shape)).astype(np.float32)) as de, \
                DeviceMaps.from_host(m.ctx, (1e-3 * rng.standard_normal(dp.shape)).astype(np.float32)) as dd, m.backward_dev(tape, de, dd) as g:
            out["gradient"] = _bits(g.maps.to_host())
    e, d = m.forward_batch(xb)
    out["infer_edge"], out["infer_dp"] = _bits(e), _bits(d)
    return out


def _check_repack(arch, precision, sizes, N=2):
    sd0 = base_sd(arch)
    sd1 = edge_case_sd(sd0, arch)
    a = fresh_model(arch, sd0, precision=precision)
    ctx = a.ctx
    b = None
    try:
        xb = np.random.default_rng(17).normal(0, 1, (1, 2, 3, 60, 64)).astype(np.float32)
        grad = a.irn_grad()
        pad0 = {"resnet50": 160, "vgg16": 160, "m7": 96}[arch]
        before = _all_bits(a, N, sizes[0], xb)
        a.load_params_dev(grad.flat_params(sd0))  # its own parameters: nothing changes
        again = _all_bits(a, N, sizes[0], xb)
        for k in before:
            assert np.array_equal(before[k], again[k]), ("reload", k)
        flat1 = grad.flat_params(sd1)
        assert np.array_equal(_bits(flat1), _bits(ref.flat_params(sd1, arch)))
        with DeviceMaps.from_host(ctx, flat1) as fd:  # a DeviceMaps is read in place
            a.load_params_dev(fd)
        b = fresh_model(arch, sd1, ctx=ctx, precision=precision)
        for S in sizes:
            got, want = _all_bits(a, N, S, xb), _all_bits(b, N, S, xb)
            assert set(got) == set(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (k, S, int((got[k] != want[k]).sum()), got[k].size)
            assert not got["tape:cat0"][..., pad0:].any()  # the padding channels of the edge concat: exact zeros
            assert got["gradient"].any() and got["edge_out"].any()
            if S == sizes[0]:  # the weights did change
                assert not np.array_equal(got["edge_out"], before["edge_out"]) and not np.array_equal(got["dp_out"], before["dp_out"])
                assert not np.array_equal(got["infer_dp"], before["infer_dp"])
    finally:
        a._release_net()
        if b is not None:
            b._release_net()
        ctx.close()


@pytest.mark.parametrize("prec", list(PRECS), ids=list(PRECS))
def test_repack_equals_creation_resnet50(prec):
    _check_repack("resnet50", PRECS[prec], (64, 68))


@pytest.mark.parametrize("arch", ["vgg16", "m7"])
def test_repack_equals_creation_thin(arch):
    _check_repack(arch, None, (64,))


# ---- 3. the trainer is the composition --------------------------------------------------------------------------------------------------
LR, WD, MAX_STEP, POWER = 0.01, 1e-4, 4, 0.9


def _trainer_case():
    rng = np.random.default_rng(9)
    return rng.normal(0, 1, (2, 3, 64, 64)).astype(np.float32), irn_loss_ref.block_labels(rng, 2, 16, 16)


def test_trainer_is_the_composition(ctx, monkeypatch, tmp_path):
    sd0 = base_sd("vgg16")
    x, label = _trainer_case()
    b = ref.boundary(sd0, "vgg16")
    m = fresh_model("vgg16", sd0, ctx=ctx)
    m2 = tr2 = tr3 = None
    tr = irn_train.IrnTrainer(m, PathIndex(5), LR, WD, MAX_STEP, power=POWER)
    try:
        assert tr.opt.sgd_momentum == WD and tr.opt.momentum == POWER  # the upstream quirk is the default
        assert PolyOptimizer(tr.grad, LR, WD, MAX_STEP, sgd_momentum=0.9).sgd_momentum == 0.9
        sd_prev, p, mom = sd0, ref.flat_params(sd0, "vgg16"), np.zeros(ref.layout(sd0, "vgg16")[1], np.float32)
        assert np.array_equal(_bits(tr.params.to_host()), _bits(p)) and not tr.mom.to_host().any()
        record = []
        for k in range(5):  # steps 3 and 4 run past max_step: the rates freeze
            assert tr.global_step == k and tr.lr == ref.poly_lrs(LR, MAX_STEP, POWER, k)
            if k == 1:  # a second step allocates nothing that it does not free
                handed, alloc0 = [], ctx.alloc

                def alloc(nbytes, pooled=False):
                    handed.append(alloc0(nbytes, pooled=pooled))
                    return handed[-1]

                monkeypatch.setattr(ctx, "alloc", alloc)
            got_l = tr.step(x, label)
            if k == 1:
                monkeypatch.undo()
                assert handed and [h.ptr for h in handed if h.ptr is not None] == []
            # the long way round: a fresh model from the previous host parameters, grad_step, the restatement on the host
            fm = fresh_model("vgg16", sd_prev, ctx=ctx)
            try:
                want_l, grads = irn_train.AffinityLoss(PathIndex(5), ctx=ctx).grad_step(fm, x, label)
                with grads:
                    g = grads.maps.to_host()
            finally:
                fm._release_net()
            assert got_l == want_l, k  # the net computes with the updated heads, to the bits
            p, mom = ref.sgd_step32(p, g, mom, b, *ref.poly_lrs(LR, MAX_STEP, POWER, k), WD, WD)
            hp, hm = tr.params_host(), tr.momentum_host()
            dp_, dm_ = _bits(ref.flat_params(hp, "vgg16")) != _bits(p), _bits(ref.flat_params(hm, "vgg16")) != _bits(mom)
            assert not dp_.any() and not dm_.any(), (k, int(dp_.sum()), int(dm_.sum()))
            assert np.isfinite(p).all() and np.abs(g).max() > 0
            assert hp["fc_dp7.0.weight"].shape == (256, 448, 1, 1)
            sd_prev = dict(sd_prev)
            sd_prev.update(hp)
            record.append((got_l, p.copy(), mom.copy()))
            print("trainer step %d: total %.6f, lr %s, max |p - p0| %.3e" % (k, got_l["total"], ref.poly_lrs(LR, MAX_STEP, POWER, k),
                                                                            np.abs(p - ref.flat_params(sd0, "vgg16")).max()))
        assert ref.poly_lrs(LR, MAX_STEP, POWER, 4) == ref.poly_lrs(LR, MAX_STEP, POWER, 3) != ref.poly_lrs(LR, MAX_STEP, POWER, 2)
        # two trainers from the same start give the same bits; save -> load -> a step = an uninterrupted step
        m2 = fresh_model("vgg16", sd0, ctx=ctx)
        with irn_train.IrnTrainer(m2, PathIndex(5), LR, WD, MAX_STEP, power=POWER) as tr2:
            for k in range(2):
                assert tr2.step(x, label) == record[k][0]
                assert np.array_equal(_bits(tr2.params.to_host()), _bits(record[k][1])) and np.array_equal(_bits(tr2.mom.to_host()), _bits(record[k][2]))
            path = str(tmp_path / "irn_trainer.npy")
            tr2.save(path)
        m2._release_net()
        tr3 = irn_train.IrnTrainer.load(path, m2, PathIndex(5), LR, WD, MAX_STEP, power=POWER)
        assert tr3.global_step == 2 and tr3.step(x, label) == record[2][0]
        assert np.array_equal(_bits(tr3.params.to_host()), _bits(record[2][1])) and np.array_equal(_bits(tr3.mom.to_host()), _bits(record[2][2]))
    finally:
        tr.close()
        if tr3 is not None:
            tr3.close()
        m._release_net()
        if m2 is not None:
            m2._release_net()


# ---- 4. dp_mean -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 17, 17), (1, 2, 1, 1), (2, 2, 128, 128)], ids=str)  # the last one is multi-block
@pytest.mark.parametrize("with_sub", [False, True])
def test_channel_mean(ctx, shape, with_sub):
    N, C, H, W = shape
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 3 + np.array([2.5, -40.0]).reshape(1, 2, 1, 1)).astype(np.float32)
    sub = np.array([0.375, -1e-3], np.float32) if with_sub else None
    want = ref.channel_mean64(x) - (sub.astype(np.float64) if with_sub else 0.0)
    outs = []
    with _guarded(ctx, x) as xd:
        for _ in range(2):
            with DeviceMaps.from_host(ctx, np.full((C + 8,), -777.25, np.float64)) as out:
                _lib.channel_mean_nchw(ctx, xd.ptr, N, C, H, W, out.ptr, sub=sub)
                o = out.to_host()
                assert (o[C:] == -777.25).all()
                outs.append(o[:C].copy())
        assert np.array_equal(_bits(_checked(xd, shape, "x")), _bits(x))  # the input and its guard
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))  # two calls: the same bits
    err = np.abs(outs[0] - want).max()
    print("channel_mean %s%s: max|d| = %.3e (bound %.3e)" % (shape, " - sub" if with_sub else "", err, 1e-12 * np.abs(x).max()))
    assert err <= 1e-12 * np.abs(x).max()


def test_fit_dp_mean_and_state_dict(ctx):
    sd0 = base_sd("vgg16")
    x, label = _trainer_case()
    m = fresh_model("vgg16", sd0, ctx=ctx)
    f = None
    try:
        with irn_train.IrnTrainer(m, PathIndex(5), LR, WD, MAX_STEP) as tr:
            tr.step(x, label)
            net = m._ensure_net()
            assert np.array_equal(net.get_mean_shift(), sd0["mean_shift.running_mean"])
            net.set_mean_shift(np.zeros(2, np.float32))  # a freshly trained model: running_mean is zeros
            batches = [net_input(2, 64), net_input(3, 64)]
            raw = []
            for xb in batches:
                e, d = m.forward_train_dev(xb)
                with e, d:
                    raw.append(d.to_host())
            first = tr.fit_dp_mean(batches)
            want = ref.dp_mean64(raw).astype(np.float32)
            print("fit_dp_mean: %s (oracle %s)" % (first, want))
            assert first.dtype == np.float32 and np.array_equal(_bits(first), _bits(want)) and np.abs(first).max() > 0
            assert np.array_equal(_bits(net.get_mean_shift()), _bits(first))
            second = tr.fit_dp_mean(batches)  # the mean shift in place is non-zero now: the mean of dp_out - shift
            assert np.array_equal(_bits(second), _bits(ref.dp_mean64(raw, first).astype(np.float32)))
            assert np.abs(second).max() <= 1e-6 * max(1.0, np.abs(first).max())
            net.set_mean_shift(first)
            sd_t = tr.state_dict()
            assert np.array_equal(sd_t["mean_shift.running_mean"], first) and set(sd_t) == set(sd0)
            assert np.array_equal(_bits(ref.flat_params(sd_t, "vgg16")), _bits(tr.params.to_host()))
            assert not np.array_equal(sd_t["fc_dp7.0.weight"], sd0["fc_dp7.0.weight"])
            assert all(np.array_equal(sd_t[k], sd0[k]) for k in sd0 if not k.startswith("fc_") and k != "mean_shift.running_mean")
            assert all(np.array_equal(m._sd[k], sd_t[k]) for k in sd_t)  # the wrapper's own copy is refreshed
        xi = np.random.default_rng(19).normal(0, 1, (2, 2, 3, 60, 64)).astype(np.float32)
        te, td = m.forward_batch(xi)
        f = fresh_model("vgg16", sd_t, ctx=ctx)
        fe, fd = f.forward_batch(xi)
        assert np.array_equal(_bits(te), _bits(fe)) and np.array_equal(_bits(td), _bits(fd))
    finally:
        m._release_net()
        if f is not None:
            f._release_net()


# ---- 5. errors before any launch ------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(ctx):
    m, sd = model("vgg16")
    mctx, net, grad = m.ctx, m._ensure_net(), m.irn_grad()
    n = grad.grad_elems
    canary = np.full((n,), CANARY, np.float32)
    other_m, _ = model("m7")
    with DeviceMaps.from_host(mctx, canary) as p, DeviceMaps.from_host(mctx, canary) as g, DeviceMaps.from_host(mctx, canary) as mo, \
            DeviceMaps.from_host(mctx, np.full((4,), -777.25, np.float64)) as out:
        good = (0.1, 1.0, 1e-4, 1e-4)

        def invalid(fn):
            with pytest.raises(_lib.WscError) as ei:
                fn()
            assert ei.value.status == _lib.WSC_ERR_INVALID

        invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, *good, elems=n - 1))
        invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, *good, ctx=ctx))  # a foreign context
        invalid(lambda: grad.sgd_step(None, g.ptr, mo.ptr, *good))
        invalid(lambda: grad.sgd_step(p.ptr, None, mo.ptr, *good))
        invalid(lambda: grad.sgd_step(p.ptr, g.ptr, None, *good))
        for i in range(4):
            for bad in (float("nan"), float("inf")):
                invalid(lambda: grad.sgd_step(p.ptr, g.ptr, mo.ptr, *[bad if j == i else v for j, v in enumerate(good)]))
        invalid(lambda: grad.load_params(p.ptr, elems=n + 1))
        invalid(lambda: grad.load_params(p.ptr, ctx=ctx))
        invalid(lambda: grad.load_params(None))
        invalid(lambda: grad.load_params(p.ptr, net=other_m._ensure_net()))  # a wsc_irn_grad of another net
        invalid(lambda: other_m.irn_grad().load_params(p.ptr, elems=other_m.irn_grad().grad_elems, net=net))
        invalid(lambda: _lib.channel_mean_nchw(mctx, None, 1, 2, 4, 4, out.ptr))
        invalid(lambda: _lib.channel_mean_nchw(mctx, p.ptr, 1, 2, 4, 4, None))
        invalid(lambda: _lib.channel_mean_nchw(mctx, p.ptr, 0, 2, 4, 4, out.ptr))
        invalid(lambda: _lib.channel_mean_nchw(mctx, p.ptr, 1, 2, 4, 4, out.ptr + 4))
        invalid(lambda: net.set_mean_shift([float("nan"), 0.0]))
        cam_sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
        cam = _lib.Net(mctx, _lib.ARCH_RESNET50_CAM, cam_sd, 20, _lib.PREC_F16)
        try:  # a CAM net has no heads and no mean shift
            invalid(lambda: grad.load_params(p.ptr, net=cam))
            invalid(lambda: cam.get_mean_shift())
            invalid(lambda: cam.set_mean_shift([0.0, 0.0]))
        finally:
            cam.close()
        mctx.sync()
        for buf in (p, g, mo):  # nothing was launched
            assert np.array_equal(_bits(buf.to_host()), _bits(canary))
        assert (out.to_host() == -777.25).all()
    with pytest.raises(ValueError):  # a trainer whose model lives on another context
        irn_train.IrnTrainer(m, PathIndex(5), LR, WD, MAX_STEP, ctx=ctx)
    with pytest.raises(ValueError):
        PolyOptimizer(grad, LR, WD, 0)
    opt = PolyOptimizer(grad, LR, WD, MAX_STEP)
    with DeviceMaps.from_host(ctx, canary) as foreign, DeviceMaps.from_host(mctx, canary) as mine:
        with pytest.raises(ValueError):
            opt.step(foreign, mine, mine)
        with pytest.raises(ValueError):
            opt.step(mine, mine, mine.to_host())
        assert opt.global_step == 0 and np.array_equal(_bits(mine.to_host()), _bits(canary))
    with pytest.raises(ValueError):
        grad.flat_params({k: v for k, v in _np_sd(sd).items() if k != "fc_dp1.1.bias"})
