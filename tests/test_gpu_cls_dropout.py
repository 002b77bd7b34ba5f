"""GPU: the dropout sites of the 01_train training step -- the BatchNorm apply with dropout and the BatchNorm gradient with a
regenerated mask (csrc/cls_grad.hip, csrc/dropout_rng.h), wsc_net_forward_cls_train_drop / wsc_net_backward_cls_drop (csrc/net.hip),
CAM.forward_train_dev(dropout=...) / backward_dev, cls_train.grad_step and ClsTrainer(drop_prob, seed) -- against the numpy Philox of
tests/seg_dropout_ref.py and the float64 oracle tests/cls_dropout_ref.py.

The per-op kernels are held to the bit: the mask is pinned to the numpy Philox (never to device code), the dropped output to
float32(y_plain * scale) of the un-dropped kernel's own output, the gradients to the un-dropped kernel run on the host-masked dy.
The whole pass at WSC_PREC_F32 and f16x3, drop_prob = 0.5: every gradient tensor within 64 R32_CHAIN_CLS_DROP max|g64| of
chain_grads_drop(float64) on the device's own downloaded tape -- the project's margin for an end-to-end backward pass (it guards the
wiring; the per-op tests hold the arithmetic).  Every test prints the figure it asserts on.

First measured on an MI355X: the worst end-to-end ratio is 4.18e-6 (VGG16 + BatchNorm, f16x3), bound 1.60e-4; the per-case
figures stand beside R32_CHAIN_CLS_DROP in tests/cls_dropout_ref.py.

Every device output of a per-op test has GUARD floats of CANARY behind it that must survive, and must be overwritten entirely."""
import functools

import numpy as np
import pytest
import torch

from tests import cls_dropout_ref as dref
from tests import cls_grad_ref as gref
from tests import net_trace_ref as nt
from tests import test_gpu_cls_grad as tcg
from tests.test_gpu_cls_grad import CANARY, EPS32, _bits, _canary, _checked, _guarded
from wsscam import _lib, cls_train
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

B = gref.B
# the smallest map; a slab of 8 channels behind a full one; the widest layer with a ragged last block of rows
OP_CASES = [(2, 64), (30, 72), (297, 1024)]
OP_PROBS = [0.5, 0.3]  # an exact scale (2), and one that rounds
SEED, STEP, SITE = 0x1234_5678_9ABC, 5, 1  # (the key's high word is in use)


def run_bn_train_drop(ctx, a, gamma, beta, run0, p, seed=SEED, step=STEP, site=SITE, y_offset=0):
    """-> (stats (C, 2), y (M, C), run (2, C)); y_offset: floats by which y_dev leaves the 16-byte grid (the scalar form)"""
    M, C = a.shape
    with _guarded(ctx, a) as ad, DeviceMaps.from_host(ctx, gamma) as gd, DeviceMaps.from_host(ctx, beta) as bd, _canary(ctx, (C, 2)) as st, \
            _canary(ctx, (M * C + y_offset,)) as y, _guarded(ctx, run0) as run:
        _lib.batch_norm_train_drop_nhwc(ctx, ad.ptr, M, C, gd.ptr, bd.ptr, gref.EPS, 0.99, True, run.ptr, st.ptr, y.ptr + 4 * y_offset, p, seed, step,
                                        site)
        yy = _checked(y, (M * C + y_offset,), "y", written=False)
        assert (yy[:y_offset] == CANARY).all() and not (yy[y_offset:] == CANARY).any()
        return _checked(st, (C, 2), "stats"), yy[y_offset:].reshape(M, C), _checked(run, (2, C), "run")


def run_bn_grad_drop(ctx, a, stats, gamma, dy, p, seed=SEED, step=STEP, site=SITE):
    M, C = a.shape
    with _guarded(ctx, a) as ad, _guarded(ctx, dy) as dd, DeviceMaps.from_host(ctx, stats) as st, DeviceMaps.from_host(ctx, gamma) as gd, \
            _canary(ctx, (M, C)) as da, _canary(ctx, (C,)) as dg, _canary(ctx, (C,)) as db:
        _lib.batch_norm_grad_drop_nhwc(ctx, ad.ptr, st.ptr, gd.ptr, dd.ptr, M, C, da.ptr, dg.ptr, db.ptr, p, seed, step, site)
        return _checked(da, (M, C), "da"), _checked(dg, (C,), "dgamma"), _checked(db, (C,), "dbeta")


def host_drop(v, p, seed=SEED, step=STEP, site=SITE):
    """(float32 where(keep, v * scale, +0.0), keep): the contract on the host, the mask from the numpy Philox"""
    return dref.dropout_f32(v, p, seed, step, site)


@pytest.mark.parametrize("p", OP_PROBS)
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "%dx%d" % c)
def test_batch_norm_train_drop(ctx, case, p):
    M, C = case
    a, gamma, beta, _, run0 = tcg.bn_case(M, C)
    stats0, y_plain, run_plain = tcg.run_bn_train(ctx, a, gamma, beta, run0)
    stats, y, run = run_bn_train_drop(ctx, a, gamma, beta, run0, p)
    assert np.array_equal(_bits(stats), _bits(stats0)) and np.array_equal(_bits(run), _bits(run_plain))
    want, keep = host_drop(y_plain, p)
    diff = int((_bits(y) != _bits(want)).sum())
    print("batch_norm_train_drop %dx%d p=%.1f: %d of %d elements differ from where(keep, y scale, 0); kept fraction %.3f" % (
        M, C, p, diff, M * C, keep.mean()))
    assert diff == 0
    assert keep.any() and not keep.all() and not np.signbit(y[~keep]).any()
    # off the 16-byte grid: the scalar form, the same bits; two calls give the same bits
    assert np.array_equal(_bits(run_bn_train_drop(ctx, a, gamma, beta, run0, p, y_offset=1)[1]), _bits(y))
    assert np.array_equal(_bits(run_bn_train_drop(ctx, a, gamma, beta, run0, p)[1]), _bits(y))
    # the counter: another step, another site and another seed are other masks; drop_prob = 0 is the un-dropped output
    for kw in ({"step": STEP + 1}, {"site": SITE - 1}, {"seed": SEED + (1 << 32)}):
        other = run_bn_train_drop(ctx, a, gamma, beta, run0, p, **kw)[1]
        assert np.array_equal(_bits(other), _bits(host_drop(y_plain, p, **kw)[0])) and not np.array_equal(other == 0, y == 0)
    assert np.array_equal(_bits(run_bn_train_drop(ctx, a, gamma, beta, run0, 0.0)[1]), _bits(y_plain))


@pytest.mark.parametrize("p", OP_PROBS)
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "%dx%d" % c)
def test_batch_norm_grad_drop(ctx, case, p):
    M, C = case
    a, gamma, beta, dy, _ = tcg.bn_case(M, C)
    mean, var, rstd, _ = gref.bn_train_ref(a, gamma, beta, EPS32)
    stats = np.stack([mean, rstd], 1).astype(np.float32)  # the taped floats
    masked, keep = host_drop(dy, p)
    want = tcg.run_bn_grad(ctx, a, stats, gamma, masked)
    got = run_bn_grad_drop(ctx, a, stats, gamma, dy, p)
    diffs = [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]
    print("batch_norm_grad_drop %dx%d p=%.1f: elements that differ from the un-dropped kernel on the host-masked dy: da %d dgamma %d dbeta %d" % (
        (M, C, p) + tuple(diffs)))
    assert diffs == [0, 0, 0]
    plain = tcg.run_bn_grad(ctx, a, stats, gamma, dy)
    assert not np.array_equal(_bits(got[2]), _bits(plain[2]))  # (it is another gradient than the un-dropped one)
    again = run_bn_grad_drop(ctx, a, stats, gamma, dy, p)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got, again))


@pytest.mark.parametrize("p", OP_PROBS)
def test_a_kept_zero_is_not_a_dropped_one(ctx, p):
    """gamma = beta = 0: every output of the channel is exactly 0.0, kept or dropped -- and dbeta is the MASKED sum of dy, which a mask
    inferred from the zeros of the output (everything "dropped") would make 0"""
    M, C, c = 30, 64, 5
    a, gamma, beta, dy, run0 = tcg.bn_case(M, C)
    gamma, beta = gamma.copy(), beta.copy()
    gamma[c] = beta[c] = 0.0
    stats, y, _ = run_bn_train_drop(ctx, a, gamma, beta, run0, p)
    assert not y[:, c].any() and not np.signbit(y[:, c]).any()
    keep = dref.keep_mask((M, C), p, SEED, STEP, SITE)
    da, dg, db = run_bn_grad_drop(ctx, a, stats, gamma, dy, p)
    want = (dy[:, c].astype(np.float64) * float(dref.scale_of(p)))[keep[:, c]].sum()
    print("kept zero p=%.1f: dbeta %.7g, the masked sum %.7g, the plain sum %.7g; %d of %d kept" % (p, db[c], want, dy[:, c].sum(), keep[:, c].sum(), M))
    assert keep[:, c].any() and not keep[:, c].all()
    assert db[c] != 0 and abs(db[c] - want) <= 2.0 ** -23 * abs(want) + M * 2.0 ** -24 * np.abs(dy[:, c]).max() * 2
    assert not da[:, c].any()  # gamma = 0: nothing goes further down
    masked = host_drop(dy, p)[0]
    assert np.array_equal(_bits(db), _bits(tcg.run_bn_grad(ctx, a, stats, gamma, masked)[2]))


def test_per_op_refusals(ctx):
    """WSC_ERR_INVALID with nothing written"""
    a, gamma, beta, dy, run0 = tcg.bn_case(30, 64)
    with DeviceMaps.from_host(ctx, a) as ad, DeviceMaps.from_host(ctx, gamma) as gd, DeviceMaps.from_host(ctx, beta) as bd, \
            _canary(ctx, (64, 2)) as st, _canary(ctx, (30, 64)) as y, _guarded(ctx, run0) as run:
        def train(M=30, C=64, p=0.5, step=STEP, site=SITE, yp=None, g=gd.ptr):
            return lambda: _lib.batch_norm_train_drop_nhwc(ctx, ad.ptr, M, C, g, bd.ptr, gref.EPS, 0.99, True, run.ptr, st.ptr,
                                                           y.ptr if yp is None else yp, p, SEED, step, site)

        def grad(C=64, p=0.5, step=STEP, site=SITE, d=ad.ptr):
            return lambda: _lib.batch_norm_grad_drop_nhwc(ctx, ad.ptr, st.ptr, gd.ptr, d, 30, C, y.ptr, st.ptr, st.ptr, p, SEED, step, site)

        calls = [train(p=1.0), train(p=-0.25), train(p=float("nan")), train(step=-1), train(step=1 << 32), train(site=-1), train(C=62),
                 train(M=1), train(g=None), train(yp=y.ptr + 2),
                 grad(p=1.0), grad(p=float("nan")), grad(step=1 << 32), grad(site=-1), grad(C=62), grad(d=None)]
        for call in calls:
            with pytest.raises(_lib.WscError) as ei:
                call()
            assert ei.value.status == _lib.WSC_ERR_INVALID
        ctx.sync()
        assert (st.to_host() == CANARY).all() and (y.to_host() == CANARY).all()
        assert np.array_equal(_bits(_checked(run, (2, 64), "run", written=False)), _bits(run0))


# ---- the whole pass ----------------------------------------------------------------------------------------------------------------
RUNS = [(c, p) for c in dref.DROP_CASES for p in ("f32", "f16x3")]


def _run_id(v):
    return gref.case_id(v) if isinstance(v, tuple) else v


def _download(m, feat, tape):
    return {"feat": feat.to_host(), "tape": {e["name"]: tape.entry(e["name"]) for e in tape.entries}, "flat": tape.maps.to_host(),
            "entries": tape.entries}


def _same_tape(one, two):
    """the entries of two passes, bit for bit (the floats between them are not written)"""
    for e in one["entries"]:
        n = (1 if e["name"].endswith(".stats") else B) * e["Ho"] * e["Wo"] * e["C"]
        if not np.array_equal(_bits(one["flat"][e["offset"]:e["offset"] + n]), _bits(two["flat"][e["offset"]:e["offset"] + n])):
            return e["name"]
    return None


@functools.lru_cache(maxsize=None)
def run_case(case, prec):
    """A dropping pass (forward, two backward calls), the pass without dropout and the pass at drop_prob = 0, everything downloaded once"""
    root, bn, pools, hw = case
    m = tcg.model(root, bn, tcg._pools_key(pools), prec)
    ctx = m.ctx
    x = gref.net_input(hw)
    out = {}
    for key, dropout in (("drop", dref.DROP), ("plain", None), ("zero", (0.0,) + dref.DROP[1:])):
        feat, tape = m.forward_train_dev(x, dropout=dropout)
        with feat, tape:
            assert ctx.range_status() == 0
            assert tape.dropout == (None if dropout is None else tuple(dropout))
            res = _download(m, feat, tape)
            dfeat = gref.case_dfeat(case, feat.shape)
            with DeviceMaps.from_host(ctx, dfeat) as dd, m.backward_dev(tape, dd) as g, m.backward_dev(tape, dd) as g2:
                res["flat_grads"] = g.maps.to_host()
                assert np.array_equal(_bits(res["flat_grads"]), _bits(g2.maps.to_host()))  # two calls: identical bits
                res["grads"], res["layout"] = g.to_state_dict(), g.layout
            if key == "drop":  # the same (seed, step) again: the same bits; another step: another mask
                feat2, tape2 = m.forward_train_dev(x, dropout=dropout)
                with feat2, tape2:
                    again = _download(m, feat2, tape2)
                assert _same_tape(res, again) is None and np.array_equal(_bits(res["feat"]), _bits(again["feat"]))
                feat3, tape3 = m.forward_train_dev(x, dropout=dropout[:2] + (dropout[2] + 1,))
                with feat3, tape3:
                    res["next_step_feat"] = feat3.to_host()
        out[key] = res
    return out


def _site_entries(root, bn, sd):
    """[(tape entry the site drops, site)] in site order (M7's site writes no entry)"""
    return [((name + ".bn") if bn else name, site) for name, site in sorted(dref.drop_sites(root, sd).items(), key=lambda kv: kv[1])]


@pytest.mark.parametrize("case,prec", RUNS, ids=_run_id)
def test_backward_vs_oracle(case, prec):
    root, bn, pools, hw = case
    sd = gref.state_dict(root, bn)
    res = run_case(case, prec)["drop"]
    dfeat = gref.case_dfeat(case, res["feat"].shape)
    want = dref.chain_grads_drop(root, sd, res["tape"], dfeat, pools, dref.DROP)
    names = gref.param_names(root, sd)
    assert [e["name"] for e in res["layout"]] == names == list(res["grads"])
    worst = gref.worst_ratio(res["grads"], want)
    print("backward_cls_drop %s %s: worst max|d| / max|g64| %.3e at %s (bound %.3e)" % (
        (gref.case_id(case), prec) + worst + (64 * dref.R32_CHAIN_CLS_DROP,)))
    for n, w in want.items():
        assert np.abs(w).max() > 0, n
        assert np.abs(res["grads"][n].astype(np.float64) - w).max() <= 64 * dref.R32_CHAIN_CLS_DROP * np.abs(w).max(), n
    # it is not the gradient of the pass without dropout
    plain = run_case(case, prec)["plain"]
    if root == "vgg16":
        assert gref.worst_ratio(plain["grads"], want)[0] > 1e-2


@pytest.mark.parametrize("case,prec", RUNS, ids=_run_id)
def test_tape(case, prec):
    """at each site the zeros lie exactly where keep_mask says dropped and the kept entries are the scaled values; every entry in
    front of the first site has the bits of the pass without dropout; the plan is unchanged"""
    root, bn, pools, hw = case
    sd = gref.state_dict(root, bn)
    runs = run_case(case, prec)
    res, plain = runs["drop"], runs["plain"]
    tape = res["tape"]
    assert res["entries"] == plain["entries"]  # no mask entry, the same offsets
    sites = _site_entries(root, bn, sd)
    assert len(sites) == (2 if root == "vgg16" else 0)
    s = float(dref.scale_of(dref.DROP[0]))
    names = [e["name"] for e in res["entries"]]
    first = names.index(sites[0][0]) if sites else len(names)
    for n in names[:first]:
        assert np.array_equal(_bits(tape[n]), _bits(plain["tape"][n])), n
    m = tcg.model(root, bn, tcg._pools_key(pools), prec)
    masks = []
    for entry, site in sites:
        T = tape[entry]
        keep = dref.keep_mask(T.shape, *dref.DROP, site)
        masks.append(keep)
        assert not T[~keep].any() and not np.signbit(T[~keep]).any(), entry  # +0.0 where dropped
        if bn:
            assert T[keep].all(), entry  # a BatchNorm output is not 0: the zeros ARE the dropped elements
            key = entry[:-3]
            C = T.shape[-1]
            a = tape[key].reshape(-1, C)
            gamma, beta = sd[dref_bn_key(root, sd, key) + ".weight"].numpy(), sd[dref_bn_key(root, sd, key) + ".bias"].numpy()
            if prec == "f32":  # the un-dropped kernel on the taped input: its y, scaled in one rounding, to the bit
                stats, y, _ = tcg.run_bn_train(m.ctx, a, gamma, beta, None)
                assert np.array_equal(_bits(stats), _bits(tape[key + ".stats"]))
                want = np.where(keep.reshape(-1, C), y * np.float32(s), np.float32(0.0)).astype(np.float32)
                assert np.array_equal(_bits(T.reshape(-1, C)), _bits(want)), entry
                print("cls drop tape %s %s %s: kept entries = fmul(y, scale) to the bit, %.3f kept" % (gref.case_id(case), prec, entry, keep.mean()))
            else:  # scale times the BatchNorm bound of test_gpu_cls_grad.py::test_tape (the planes' split included)
                mean, var, rstd, y64 = gref.bn_train_ref(a, gamma, beta, EPS32)
                b_y = tcg.bn_bounds(a, gamma, mean, var, rstd, y64)[2] + 2.0 ** -22 * np.abs(y64) + 2.0 ** -25
                e = np.abs(T.reshape(-1, C).astype(np.float64) - s * y64)[keep.reshape(-1, C)]
                ratio = float((e / (s * b_y[keep.reshape(-1, C)])).max())
                print("cls drop tape %s %s %s: kept entries, worst err / (scale x bound) %.3f" % (gref.case_id(case), prec, entry, ratio))
                assert ratio <= 1.0, entry
        else:  # a post-ReLU site: kept = scale x the convolution of the entry in front, at the suite's per-precision conv bound
            prev = names[names.index(entry) - 1]
            w = sd[entry + ".weight"]
            ly = nt.Layer(entry, "conv", nt.plain_conv(w, sd[entry + ".bias"], None, None), (0, nt.NONE, nt.NONE), K=int(np.prod(w.shape[1:])))
            xt = torch.from_numpy(np.ascontiguousarray(tape[prev])).double().permute(0, 3, 1, 2)
            ref, A, S = [v.numpy().transpose(0, 2, 3, 1) for v in ly.fn(xt)]
            bound = nt.asserted_bound(prec, ly, ref, A, S)[0]
            e = np.abs(T.astype(np.float64) / s - ref)[keep]  # (scale = 2: the division is exact)
            ratio = float((e / np.maximum(bound[keep], 1e-300)).max())
            print("cls drop tape %s %s %s: kept entries / scale against the float64 conv, worst err / bound %.3f" % (gref.case_id(case), prec, entry, ratio))
            assert ratio <= 1.0 and (T[keep] > 0).any(), entry
    if root == "vgg16":
        assert (masks[0] != masks[1]).any()  # two sites of one pass: two masks
        assert np.array_equal(_bits(res["feat"]), _bits(tape[sites[1][0]]))  # feat is the dropped output of site 1
    else:  # M7: every entry is the un-dropped pass's; feat = pool -> mask of the last one, exactly
        last = tape[names[-2] if bn else names[-1]]
        pooled = gref._nhwc(dref.head_pool_t(gref._nchw(last, torch.float32), pools))
        want, keep = dref.dropout_f32(pooled, *dref.DROP, dref.M7_SITE)
        assert res["feat"].shape == pooled.shape != plain["feat"].shape
        assert np.array_equal(_bits(res["feat"]), _bits(want))
        assert m._ensure_net().cls_feat_dims(hw[0], hw[1], True) == pooled.shape[1:3]
    assert not np.array_equal(res["next_step_feat"] == 0, res["feat"] == 0)  # another step: another mask


def dref_bn_key(root, sd, key):
    return next(b for _, n, b in gref.stack_ops(root, sd) if n == key)


@pytest.mark.parametrize("case,prec", RUNS, ids=_run_id)
def test_drop_prob_zero_is_the_existing_pass(case, prec):
    root, bn, pools, hw = case
    runs = run_case(case, prec)
    zero, plain = runs["zero"], runs["plain"]
    assert zero["feat"].shape == plain["feat"].shape  # (M7: the un-pooled map)
    assert np.array_equal(_bits(zero["feat"]), _bits(plain["feat"])) and _same_tape(zero, plain) is None
    assert np.array_equal(_bits(zero["flat_grads"]), _bits(plain["flat_grads"])) and np.abs(plain["flat_grads"]).max() > 0
    net = tcg.model(root, bn, tcg._pools_key(pools), prec)._ensure_net()
    assert net.cls_feat_dims(hw[0], hw[1], False) == net.cam_size_hw(hw[0], hw[1]) == plain["feat"].shape[1:3]


def test_m7_dropped_zero_wins_the_maximum():
    """a BatchNorm net whose last beta is strongly negative on one channel: every kept value of the channel is negative, the dropped
    +0.0 is the maximum the loss head takes; its gradient lands on dropped elements only, and nothing reaches the channel's
    parameters.  The whole result agrees with the oracle on the device's tape and the device's d loss / d feat."""
    from wsscam.net import m7_cam

    case, c = ("m7", True, None, (40, 24)), 3
    sd = {k: v.clone() for k, v in gref.state_dict("m7", True).items()}
    sd["m7.layer3_p1.8.bias"][c] = -50.0
    m = m7_cam.CAM(None, "voc12", "", 20, None, precision=_lib.PREC_F32)
    m.load_state_dict(sd)
    m.eval().cuda(0)
    try:
        ctx = m.ctx
        loss = cls_train.ClsLoss(ctx, "max", 20)
        targets = (np.random.default_rng(8).random((B, 20)) < 0.3).astype(np.float32)
        w, bias = m.classifier_params()
        feat, tape = m.forward_train_dev(gref.net_input(case[3]), dropout=dref.DROP)
        with feat, tape:
            metrics, head = loss.grad_step(feat, w, bias, targets)
            with head.feat, head.w, head.bias, m.backward_dev(tape, head.feat) as g:
                f, dfeat, grads = feat.to_host(), head.feat.to_host(), g.to_state_dict()
                host_tape = {e["name"]: tape.entry(e["name"]) for e in tape.entries}
        keep = dref.keep_mask(f.shape, *dref.DROP, dref.M7_SITE)
        assert dfeat.shape == f.shape and (f[..., c] <= 0).all() and (f[..., c].reshape(B, -1).max(1) == 0).all()
        assert np.abs(dfeat[..., c]).max() > 0 and not dfeat[..., c][keep[..., c]].any()  # the loss's gradient sits on dropped zeros
        for n in ("m7.layer3_p1.8.weight", "m7.layer3_p1.8.bias", "m7.layer3_p1.6.bias"):
            assert grads[n][c] == 0 and np.abs(grads[n]).max() > 0, n
        assert not grads["m7.layer3_p1.6.weight"][c].any()
        want = dref.chain_grads_drop("m7", sd, host_tape, dfeat, None, dref.DROP)
        worst = gref.worst_ratio(grads, want)
        print("m7 dropped zero wins: loss %.6f, worst max|d| / max|g64| %.3e at %s (bound %.3e)" % ((metrics["loss"],) + worst + (64 * dref.R32_CHAIN_CLS_DROP,)))
        assert all(np.abs(grads[n].astype(np.float64) - v).max() <= 64 * dref.R32_CHAIN_CLS_DROP * np.abs(v).max() for n, v in want.items())
    finally:
        m._release_net()


def test_refusals_before_any_launch(ctx):
    """the dropout arguments, a wrong feat_elems / dfeat_elems and what the un-dropped entry points refuse: WSC_ERR_INVALID, and the
    outputs keep their canaries"""
    case = ("m7", True, None, (40, 24))
    m = tcg.model("m7", True, None, "f32")
    mctx, net = m.ctx, m._ensure_net()
    H, W = case[3]
    entries, elems = net.cls_tape_plan(B, H, W)
    (h, w), (hp, wp) = net.cls_feat_dims(H, W, False), net.cls_feat_dims(H, W, True)
    assert (hp, wp) == (h // 2, w // 2) and (h, w) == net.cam_size_hw(H, W)
    n_full, n_pool = B * h * w * 256, B * hp * wp * 256
    grad = m.cls_grad()
    with DeviceMaps.from_host(mctx, gref.net_input((H, W))) as xd, _canary(mctx, (elems,)) as tape, _canary(mctx, (n_full,)) as feat, \
            _canary(mctx, (grad.grad_elems,)) as out, DeviceMaps.from_host(mctx, np.zeros((n_full,), np.float32)) as dfeat:
        def fwd(n=n_pool, p=0.5, step=3, te=elems, **kw):
            return lambda: net.forward_cls_train_drop(xd.ptr, B, H, W, tape.ptr, te, feat.ptr, n, p, 7, step, **kw)

        def bwd(n=n_pool, p=0.5, step=3, te=elems, **kw):
            return lambda: grad.backward_drop(B, H, W, tape.ptr, te, dfeat.ptr, n, out.ptr, p, 7, step, **kw)

        bad = [fwd(p=1.0), fwd(p=-0.5), fwd(p=float("nan")), fwd(step=-1), fwd(step=1 << 32), fwd(n=n_full), fwd(n=n_pool, p=0.0),
               fwd(n=n_pool - 1), fwd(te=elems - 64), fwd(keep=1.25),
               bwd(p=1.0), bwd(p=float("nan")), bwd(step=1 << 32), bwd(n=n_full), bwd(n=n_pool, p=0.0), bwd(te=elems - 64),
               bwd(grad_elems=grad.grad_elems - 1), bwd(ctx=ctx)]
        for call in bad:
            with pytest.raises(_lib.WscError) as ei:
                call()
            assert ei.value.status == _lib.WSC_ERR_INVALID
        mctx.sync()
        for buf, n in ((tape, elems), (feat, n_full), (out, grad.grad_elems)):
            assert (_checked(buf, (n,), "refused", written=False) == CANARY).all()  # nothing was launched
        # the Python layer
        with pytest.raises(ValueError):
            m.forward_train_dev(gref.net_input((H, W)), keep=False, dropout=dref.DROP)
        et = cls_train.ClsTape(DeviceMaps(mctx, (elems,), np.float32, tape.buf), entries, B, H, W, dref.DROP)
        with DeviceMaps(mctx, (B, h, w, 256), np.float32) as unpooled, pytest.raises(ValueError):
            m.backward_dev(et, unpooled)  # a dropping M7 tape takes the pooled shape
    with pytest.raises(_lib.WscError) as ei:
        net.cls_feat_dims(0, W, True)
    assert ei.value.status == _lib.WSC_ERR_INVALID


@pytest.mark.parametrize("root", ["vgg16", "m7"])
def test_nan_in_the_input_never_leaves_as_finite_gradients(root):
    """DESIGN.md section 5.1's rule, as tests/test_gpu_cls_grad.py holds it without dropout: the range status is the contract (the
    input door raises the flag in every precision), and behind it every conv and BatchNorm WEIGHT gradient is NaN all the same -- a
    dropped NaN becomes 0.0 on the tape, the kept ones stay"""
    hw = (33, 33) if root == "vgg16" else (40, 24)
    case = (root, True, None, hw)
    m = tcg.model(root, True, None, "f32")
    ctx = m.ctx
    x = gref.net_input(hw).copy()
    x[1, 2, 17, 5] = np.nan
    raised, grads = None, None
    try:
        feat, tape = m.forward_train_dev(x, bn_keep=None, dropout=dref.DROP)
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
    print("NaN input with dropout, %s: status %s, %d of %d tensors not finite" % (
        root, raised, sum(1 for v in grads.values() if not np.isfinite(v).all()), len(grads)))
    assert raised == _lib.WSC_ERR_RANGE
    assert all(not np.isfinite(v).all() for n, v in grads.items() if n.endswith(".weight"))


# ---- Python: grad_step and the trainer ---------------------------------------------------------------------------------------------
def test_grad_step_with_dropout():
    case = ("m7", True, None, (40, 24))
    m = tcg.model("m7", True, None, "f16x3")
    ctx = m.ctx
    x = gref.net_input(case[3])
    targets = (np.random.default_rng(8).random((B, 20)) < 0.3).astype(np.float32)
    loss = cls_train.ClsLoss(ctx, "max", 20)
    w, bias = m.classifier_params()
    feat, tape = m.forward_train_dev(x, dropout=dref.DROP)
    with feat, tape:
        want_metrics, head = loss.grad_step(feat, w, bias, targets)
        with head.feat, head.w, head.bias, m.backward_dev(tape, head.feat) as want:
            want_flat, want_head = want.maps.to_host(), [v.to_host() for v in head]
    metrics, head, grads = cls_train.grad_step(m, loss, x, targets, dropout=dref.DROP)
    with head.feat, head.w, head.bias, grads:
        assert metrics == want_metrics
        assert all(np.array_equal(_bits(a.to_host()), _bits(b)) for a, b in zip(head, want_head))
        assert np.array_equal(_bits(grads.maps.to_host()), _bits(want_flat)) and np.abs(want_flat).max() > 0
        assert tuple(head.feat.shape) == (B,) + m._ensure_net().cls_feat_dims(40, 24, True) + (256,)
    plain_metrics, head, grads = cls_train.grad_step(m, loss, x, targets)
    with head.feat, head.w, head.bias, grads:
        assert plain_metrics != metrics
    print("grad_step with dropout: loss %.6f, without %.6f" % (metrics["loss"], plain_metrics["loss"]))


@pytest.mark.parametrize("net", ["vgg16-bn", "m7-keras"])
def test_trainer_resumes_bit_for_bit(ctx, net, tmp_path):
    """ClsTrainer(drop_prob=0.5, seed=7): three steps, save, load, two more = five uninterrupted steps, bit for bit -- parameters,
    momentum and running statistics; the file carries seed and drop_prob, and an explicit keyword wins"""
    from tests import test_gpu_cls_sgd as tcs

    root, bn, pools = tcs.NETS[net]
    sd0 = tcs.base_sd(net)
    x, targets, sw = tcs._trainer_case()
    prec = _lib.PREC_F16X3
    lrs = (0.01, 0.01, 0.004, 0.004, 0.002)
    made = []

    def fresh(sd=None):
        made.append(tcs.fresh_model(net, sd0, prec, ctx=ctx) if sd is None else sd)
        return made[-1]

    def state(tr):
        run = tr.model.bn_running()
        return [tr.params.to_host(), tr.mom.to_host()] + [run[k] for k in sorted(run)]

    try:
        with cls_train.ClsTrainer(fresh(), tcs.POOL[root], tcs.C, drop_prob=0.5, seed=7) as tr:
            losses = [tr.step(x, targets, lr, sw)["loss"] for lr in lrs]
            want = state(tr)
        path = str(tmp_path / "drop_trainer.npy")
        with cls_train.ClsTrainer(fresh(), tcs.POOL[root], tcs.C, drop_prob=0.5, seed=7) as tr:
            first = [tr.step(x, targets, lr, sw)["loss"] for lr in lrs[:3]]
            tr.save(path)
        saved = np.load(path, allow_pickle=True).item()["__step__"]
        assert saved == {"global_step": 3, "seed": 7, "drop_prob": 0.5}
        cls = type(made[0])
        m3 = fresh(cls(None, "voc12", "", tcs.C, None, precision=prec, pooling=None if pools is None else list(pools)))
        m3._ctx = ctx
        with cls_train.ClsTrainer.load(path, m3, tcs.POOL[root], tcs.C) as tr:
            assert (tr.global_step, tr.seed, tr.drop_prob) == (3, 7, 0.5)
            rest = [tr.step(x, targets, lr, sw)["loss"] for lr in lrs[3:]]
            got = state(tr)
        assert first + rest == losses
        diffs = [int((_bits(a) != _bits(b)).sum()) for a, b in zip(got, want)]
        print("trainer with dropout %s: losses %s; elements that differ after the resume: %s" % (net, ["%.6f" % v for v in losses], diffs))
        assert not any(diffs)
        # an explicit keyword wins over the file; a file without the two keys loads as 0
        m4 = fresh(cls(None, "voc12", "", tcs.C, None, precision=prec, pooling=None if pools is None else list(pools)))
        m4._ctx = ctx
        with cls_train.ClsTrainer.load(path, m4, tcs.POOL[root], tcs.C, seed=9, drop_prob=0.25) as tr:
            assert (tr.global_step, tr.seed, tr.drop_prob) == (3, 9, 0.25)
        old = np.load(path, allow_pickle=True).item()
        old["__step__"] = {"global_step": 3}
        with open(path, "wb") as fh:
            np.save(fh, old, allow_pickle=True)
        m5 = fresh(cls(None, "voc12", "", tcs.C, None, precision=prec, pooling=None if pools is None else list(pools)))
        m5._ctx = ctx
        with cls_train.ClsTrainer.load(path, m5, tcs.POOL[root], tcs.C) as tr:
            assert (tr.global_step, tr.seed, tr.drop_prob) == (3, 0, 0.0)
            plain = tr.step(x, targets, lrs[3], sw)["loss"]
            tr.save(path)  # a trainer without dropout writes the file it always wrote
        assert np.load(path, allow_pickle=True).item()["__step__"] == {"global_step": 4}
        assert plain != rest[0]  # without dropout it is another step
        with pytest.raises(ValueError):
            cls_train.ClsTrainer(made[0], tcs.POOL[root], tcs.C, drop_prob=1.0)
    finally:
        for mm in made:
            mm._release_net()
