"""GPU: the IRNet training loss on the device (csrc/irn_loss.hip, wsc_irn_aff_loss; irn_train.AffinityLoss) against the float64
oracle tests/irn_loss_ref.py, and Net.forward in training mode (wsc_net_forward_edge_raw) against oracle/irn_ref.py.

Bounds (DESIGN.md section 5 carries the measured errors next to them):
  pair counts  exact.
  loss values  |got - want| <= max(1e-10, 4 N 2^-53) * sum|terms|, N the number of terms behind the value: both sides work in
               double on identical float32 inputs, so they differ by the order of their sums.
  gradients    |got - want| <= 2^-23 |want| + 1e-10 max|want|: one float32 rounding of a double value plus double-level
               cancellation (a pixel's gradient adds positive-pair and negative-pair terms of opposite sign).
The random cases carry no tied path maximum (asserted); the tie case is compared with the same bounds against the oracle's
max_pool2d placement -- a misplaced gradient is off by its whole value."""
import numpy as np
import pytest
import torch

from oracle import irn_ref
from tests import irn_loss_ref as ref
from wsscam import _lib, irn_train
from wsscam.misc.indexing import PathIndex
from wsscam.net import m7_irn, vgg16_irn
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

CANARY = np.float32(-777.25)
GUARD = 256  # canary floats behind each output
N_SLOTS = len(ref.KEYS)


@pytest.fixture(scope="module")
def oracle():
    """case -> (inputs, oracle result): computed once, shared, never modified"""
    out = {}
    for case in ref.CASES:
        inputs = ref.make_case(case)
        out[case] = (inputs, ref.tensor_form(*inputs, case[0]))
    return out


def raw_call(ctx, edge, dp, label, B, h, w, dirs, start, yx, D, rf, valid_below, loss, g_edge, g_dp):
    """wsc_irn_aff_loss with nothing checked on the way (a table may be None)"""
    _lib.check(ctx._lib.wsc_irn_aff_loss(ctx.h, _lib._ptr(edge), _lib._ptr(dp), _lib._ptr(label), B, h, w, _lib._ptr(dirs),
                                         _lib._ptr(start), _lib._ptr(yx), D, rf, valid_below, _lib._ptr(loss), _lib._ptr(g_edge),
                                         _lib._ptr(g_dp)))


def run(ctx, edge, dp, label, radius, want=("edge", "dp"), valid_below=21):
    """one wsc_irn_aff_loss on uploaded arrays -> (loss float64 [10], g_edge, g_dp); the three outputs start canary-filled with
    GUARD more canaries behind them, the guards are checked here, and only a requested gradient is handed to the call"""
    B, h, w = edge.shape
    pi = PathIndex(radius)
    dirs, start, yx = pi.device_tables()
    n = B * h * w
    with DeviceMaps.from_host(ctx, edge) as e, DeviceMaps.from_host(ctx, dp) as d, DeviceMaps.from_host(ctx, label) as lab, \
            DeviceMaps.from_host(ctx, np.full(2 * N_SLOTS + GUARD, CANARY)) as loss, \
            DeviceMaps.from_host(ctx, np.full(n + GUARD, CANARY)) as ge, DeviceMaps.from_host(ctx, np.full(2 * n + GUARD, CANARY)) as gd:
        _lib.irn_aff_loss(ctx, e.ptr, d.ptr, lab.ptr, B, h, w, dirs, start, yx, pi.radius_floor, valid_below, loss.ptr,
                          grad_edge_dev=ge.ptr if "edge" in want else None, grad_dp_dev=gd.ptr if "dp" in want else None)
        lo, a, b = loss.to_host(), ge.to_host(), gd.to_host()
    assert (lo[2 * N_SLOTS:] == CANARY).all() and (a[n:] == CANARY).all() and (b[2 * n:] == CANARY).all()
    return lo[:2 * N_SLOTS].view(np.float64).copy(), a[:n].reshape(B, h, w), b[:2 * n].reshape(B, 2, h, w)


def check_losses(loss, want):
    """-> the largest |err| / sum|terms|"""
    worst = 0.0
    for k, name in enumerate(ref.KEYS):
        err = abs(loss[k] - want["loss"][name])
        if name.startswith("n_"):
            assert loss[k] == want["loss"][name], (name, loss[k], want["loss"][name])
            continue
        mag = want["mag"][name]
        if mag > 0:
            worst = max(worst, err / mag)
        assert err <= ref.loss_bound(mag, want["terms"][name]), (name, loss[k], want["loss"][name], mag)
    return worst


def grad_excess(got, want):
    """max of |got - want| - (2^-23 |want| + 1e-10 max|want|): <= 0 passes; and the largest error relative to max|want|"""
    err = np.abs(got.astype(np.float64) - want)
    top = np.abs(want).max()
    return float((err - (2.0 ** -23 * np.abs(want) + 1e-10 * top)).max()), float(err.max() / top) if top > 0 else 0.0


@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_losses_and_gradients_vs_oracle(ctx, oracle, case):
    (edge, dp, label), want = oracle[case]
    assert want["tied"] == 0.0
    if case != ref.CASES[0]:  # (the single source has four pairs)
        assert min(want["loss"][k] for k in ("n_bg", "n_fg", "n_neg")) > 0
    loss, ge, gd = run(ctx, edge, dp, label, case[0])
    worst = check_losses(loss, want)
    ex_e, rel_e = grad_excess(ge, want["g_edge"])
    ex_d, rel_d = grad_excess(gd, want["g_dp"])
    print("irn_aff_loss %s: pairs %d / %d / %d, loss max |err| / sum|terms| %.3g; g_edge max |err| / max|g| %.3g, g_dp %.3g"
          % (case, loss[7], loss[8], loss[9], worst, rel_e, rel_d))
    assert np.isfinite(ge).all() and np.isfinite(gd).all()
    assert ex_e <= 0 and ex_d <= 0
    # pixels that no pair touches hold +0.0
    assert not np.signbit(ge[want["g_edge"] == 0]).any() and not np.signbit(gd[want["g_dp"] == 0]).any()
    # a second call: the same bits
    loss2, ge2, gd2 = run(ctx, edge, dp, label, case[0])
    assert loss.tobytes() == loss2.tobytes() and ge.tobytes() == ge2.tobytes() and gd.tobytes() == gd2.tobytes()
    # either gradient alone has the bits it has beside the other; an unrequested buffer keeps its canary
    loss_e, ge_e, gd_e = run(ctx, edge, dp, label, case[0], want=("edge",))
    loss_d, ge_d, gd_d = run(ctx, edge, dp, label, case[0], want=("dp",))
    loss_n, ge_n, gd_n = run(ctx, edge, dp, label, case[0], want=())
    assert loss_e.tobytes() == loss_d.tobytes() == loss_n.tobytes() == loss.tobytes()
    assert np.array_equal(ge_e, ge) and (gd_e == CANARY).all()
    assert np.array_equal(gd_d, gd) and (ge_d == CANARY).all()
    assert (ge_n == CANARY).all() and (gd_n == CANARY).all()


def test_ties_go_to_the_first_pixel_and_abs_has_no_gradient_at_zero(ctx):
    case = (5, 2, 16, 20)
    edge, dp, label = ref.make_case(case, integer=True)
    want = ref.tensor_form(edge, dp, label, 5)
    assert want["tied"] > 0.10
    assert min(want["loss"][k] for k in ("n_bg", "n_fg", "n_neg")) > 0
    loss, ge, gd = run(ctx, edge, dp, label, 5)
    check_losses(loss, want)
    assert grad_excess(ge, want["g_edge"])[0] <= 0 and grad_excess(gd, want["g_dp"])[0] <= 0


def test_saturated_logits_stay_finite(ctx):
    case = (5, 2, 16, 20)
    _, dp, label = ref.make_case(case)
    rng = np.random.default_rng(3)
    for scale in (40.0, 800.0):
        edge = (scale * rng.choice([-1.0, 1.0], (2, 16, 20))).astype(np.float32)
        loss, ge, gd = run(ctx, edge, dp, label, 5)
        assert np.isfinite(loss).all() and np.isfinite(ge).all() and np.isfinite(gd).all()
        assert min(loss[7:]) > 0 and loss[3] > 0 and loss[2] > 0


def test_degenerate_labels(ctx):
    case = (5, 2, 16, 20)
    edge, dp, _ = ref.make_case(case)
    zero = bytes(8 * N_SLOTS)
    for lab_value, vb in ((255, 21), (21, 21), (7, 7)):  # ignore; valid_below itself counts as ignore
        loss, ge, gd = run(ctx, edge, dp, np.full((2, 16, 20), lab_value, np.uint8), 5, valid_below=vb)
        assert loss.tobytes() == zero and ge.tobytes() == bytes(ge.nbytes) and gd.tobytes() == bytes(gd.nbytes)
    label = np.zeros((2, 16, 20), np.uint8)
    want = ref.tensor_form(edge, dp, label, 5)
    loss, ge, gd = run(ctx, edge, dp, label, 5)
    check_losses(loss, want)
    named = dict(zip(ref.KEYS, loss))
    assert named["n_bg"] == 2 * (16 - 4) * (20 - 8) * 34 and named["n_fg"] == named["n_neg"] == 0
    assert named["pos_fg"] == named["neg"] == named["dp_fg"] == 0 and named["pos_bg"] > 0 and named["dp_bg"] > 0
    assert grad_excess(ge, want["g_edge"])[0] <= 0 and grad_excess(gd, want["g_dp"])[0] <= 0


def test_batch_is_the_sum_of_its_images(ctx, oracle):
    """counts and sums, not the quotients: S = value * denominator of every mean"""
    case = (5, 3, 33, 37)
    (edge, dp, label), want = oracle[case]
    dens = {"pos_bg": ("n_bg", 1), "pos_fg": ("n_fg", 1), "neg": ("n_neg", 1), "dp_fg": ("n_fg", 2), "dp_bg": ("n_bg", 2)}

    def sums(loss):
        named = dict(zip(ref.KEYS, loss))
        return named, {k: named[k] * (m * named[n] + 1e-5) for k, (n, m) in dens.items()}

    whole, s_whole = sums(run(ctx, edge, dp, label, 5, want=())[0])
    parts = [sums(run(ctx, edge[b:b + 1], dp[b:b + 1], label[b:b + 1], 5, want=())[0]) for b in range(3)]
    for k in ("n_bg", "n_fg", "n_neg"):
        assert sum(p[0][k] for p in parts) == whole[k]
    for k in dens:
        # a quotient and a product round twice more per value; the terms are positive, so the sums are their own magnitudes
        assert abs(sum(p[1][k] for p in parts) - s_whole[k]) <= ref.loss_bound(abs(s_whole[k]), want["terms"][k]) + 8 * 2.0 ** -53 * abs(s_whole[k]), k


def test_arguments_are_checked_before_any_launch(ctx):
    B, h, w, rf = 1, 9, 11, 2
    dirs, start, yx = PathIndex(3).device_tables()
    D = len(dirs)
    n = B * h * w
    # [loss | g_edge | g_dp | edge | dp | label], all canary
    with DeviceMaps.from_host(ctx, np.full(32 + 7 * n, CANARY, np.float32)) as buf:
        loss, ge, gd = buf.ptr, buf.ptr + 128, buf.ptr + 128 + 4 * n
        edge, dp, lab = buf.ptr + 128 + 12 * n, buf.ptr + 128 + 16 * n, buf.ptr + 128 + 24 * n

        def call(**kw):
            a = dict(edge=edge, dp=dp, label=lab, B=B, h=h, w=w, dirs=dirs, start=start, yx=yx, D=D, rf=rf, valid_below=21, loss=loss,
                     g_edge=ge, g_dp=gd)
            a.update(kw)
            raw_call(ctx, *[a[k] for k in ("edge", "dp", "label", "B", "h", "w", "dirs", "start", "yx", "D", "rf", "valid_below", "loss",
                                           "g_edge", "g_dp")])

        far_dir, far_path, side_path = dirs.copy(), yx.copy(), yx.copy()
        far_dir[3, 0] = rf + 1
        far_path[5, 0] = -1
        side_path[7, 1] = -(rf + 1)
        empty = start.copy()
        empty[2] = empty[1]
        bad = [
            (dict(h=rf), "h=2"), (dict(w=2 * rf), "w=4"), (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(D=0), "D=0"),
            (dict(rf=17), "radius_floor=17"), (dict(valid_below=0), "valid_below=0"),
            (dict(dirs=far_dir), "dirs_host"), (dict(yx=far_path), "path_yx_host"), (dict(yx=side_path), "path_yx_host"),
            (dict(start=empty), "path_start_host"),
            (dict(edge=None), "edge_dev"), (dict(dp=None), "dp_dev"), (dict(label=None), "label_dev"), (dict(loss=None), "loss_dev"),
            (dict(dirs=None), "dirs_host"), (dict(start=None), "path_start_host"), (dict(yx=None), "path_yx_host"),
            (dict(g_edge=edge), "grad_edge_dev overlaps edge_dev"), (dict(g_dp=dp + 4), "grad_dp_dev overlaps dp_dev"),
            (dict(g_edge=lab), "grad_edge_dev overlaps label_dev"), (dict(g_dp=ge), "grad_edge_dev overlaps grad_dp_dev"),
        ]
        for kw, word in bad:
            with pytest.raises(_lib.WscError) as ei:
                call(**kw)
            assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (word, str(ei.value))
        ctx.sync()
        assert (buf.to_host() == CANARY).all()  # nothing was launched


def test_affinity_loss_is_that_call(ctx, oracle):
    case = (5, 2, 16, 20)
    (edge, dp, label), _ = oracle[case]
    loss, ge, gd = run(ctx, edge, dp, label, 5)
    al = irn_train.AffinityLoss(PathIndex(5), ctx=ctx)
    losses, g_e, g_d = al(edge[:, None], dp, label)  # (B, 1, h, w), as the network hands it out
    with g_e, g_d:
        assert g_e.shape == (2, 1, 16, 20) and g_d.shape == dp.shape
        assert np.array_equal(g_e.to_host()[:, 0], ge) and np.array_equal(g_d.to_host(), gd)
    assert [losses[k] for k in ref.KEYS] == loss.tolist() and all(isinstance(v, float) for v in losses.values())
    with DeviceMaps.from_host(ctx, edge) as e, DeviceMaps.from_host(ctx, dp) as d, DeviceMaps.from_host(ctx, label) as lab:
        l2, none_e, none_d = al(e, d, lab, want_grad=False)  # device maps are read in place and stay the caller's
        assert l2 == losses and none_e is None and none_d is None and e.ptr is not None
        for fn, word in ((lambda: al(e, dp[:, :1], lab), "dp_out"), (lambda: al(e, d, label[:1]), "label"),
                         (lambda: al(edge[0], dp, label), "edge_out"), (lambda: al(e, d, e), "label")):
            with pytest.raises(ValueError) as ei:
                fn()
            assert word in str(ei.value)
    with pytest.raises(ValueError):
        irn_train.AffinityLoss(PathIndex(5), valid_below=0, ctx=ctx)
    big = np.arange(8 * 12, dtype=np.uint8).reshape(8, 12)
    small = irn_train.reduce_label(big)
    assert small.shape == (2, 3) and small.dtype == np.uint8 and np.array_equal(small, irn_train.imutils.pil_rescale(big, 0.25, 0))


def thin_net(arch):
    """the thin IRNet test nets of tests/test_gpu_irn.py at S = 64, with that file's tolerances (edge, displacement)"""
    if arch == "vgg16":
        sd = irn_ref.make_vgg16_irn_state_dict(seed=2)
        m = vgg16_irn.EdgeDisplacement(None, "voc12", "", 20, None, crop_size=64, stride=4, precision=_lib.PREC_F16X3)
    else:
        sd = irn_ref.make_m7_irn_state_dict(seed=4)
        m = m7_irn.EdgeDisplacement(None, "voc12", "", 20, None, crop_size=64, stride=4)
    m.load_state_dict(sd)
    m.eval().cuda(0)
    return m, sd, (2e-4, 2e-3)


@pytest.mark.parametrize("arch", ["vgg16", "m7"])
def test_forward_edge_raw(arch):
    m, sd, (te, td) = thin_net(arch)
    rng = np.random.default_rng(8)
    img = rng.normal(0, 1, (3, 64, 64)).astype(np.float32)
    x = np.ascontiguousarray(np.stack([img, img[:, :, ::-1]]))  # [x, flip(x)]
    (He, We), (Hd, Wd) = m._ensure_net().edge_size(64)
    assert (Hd, Wd) == (16, 16) and (He, We) == ((32, 32) if arch == "m7" else (16, 16))
    edge, dp = m.forward_train_dev(x)
    with edge, dp:
        assert edge.shape == (2, He, We) and dp.shape == (2, 2, Hd, Wd)
        e, d = edge.to_host(), dp.to_host()
    # against the torch restatement; MeanShift is the identity while training, the restatement subtracts it
    with torch.no_grad():
        we, wd = irn_ref.irn_net_forward(torch.from_numpy(x), sd, arch)
        wd = wd + sd["mean_shift.running_mean"].view(1, 2, 1, 1)
    we, wd = we.numpy()[:, 0], wd.numpy()
    # the existing edge test bounds sigmoid(edge) by `te`; the logits get the relative form the displacement bound has
    assert np.abs(1 / (1 + np.exp(-e.astype(np.float64))) - 1 / (1 + np.exp(-we.astype(np.float64)))).max() <= te
    assert np.abs(e - we).max() <= te * max(1.0, float(np.abs(we).max())), np.abs(e - we).max()
    assert np.abs(d - wd).max() <= td * max(1.0, float(np.abs(wd).max())), np.abs(d - wd).max()
    # its outputs through wsc_irn_edge_finish are wsc_net_forward_edge's, bit for bit
    ctx = m.ctx
    ms = sd["mean_shift.running_mean"].numpy()
    with DeviceMaps.from_host(ctx, e) as e_dev, DeviceMaps.from_host(ctx, np.ascontiguousarray(d.transpose(0, 2, 3, 1))) as d_dev:
        fe, fd = _lib.irn_edge_finish(ctx, e_dev.ptr, He, We, d_dev.ptr, Hd, Wd, 1, 16, 16, ms[0], ms[1])
        got_e, got_d = ctx.to_host(fe, (1, 16, 16), np.float32), ctx.to_host(fd, (2, 16, 16), np.float32)
        fe.free()
        fd.free()
    want_e, want_d = m.forward(x)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_d, want_d)
    # device input, read in place
    with DeviceMaps.from_host(ctx, x) as xd:
        e2, d2 = m.forward_train_dev(xd)
        with e2, d2:
            assert np.array_equal(e2.to_host(), e) and np.array_equal(d2.to_host(), d) and xd.ptr is not None
    with pytest.raises(ValueError):
        m.forward_train_dev(x[:, :, :, :32])


def test_loss_step_is_the_composition_of_its_parts(ctx):
    m, sd, _ = thin_net("vgg16")
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, (2, 3, 64, 64)).astype(np.float32)
    label = ref.block_labels(rng, 2, 16, 16)
    al = irn_train.AffinityLoss(PathIndex(5), ctx=m.ctx)
    edge, dp = m.forward_train_dev(x)
    with edge, dp:
        want, w_e, w_d = al(edge, dp, label)
        with w_e, w_d:
            we, wd, e_host, d_host = w_e.to_host(), w_d.to_host(), edge.to_host(), dp.to_host()
    assert min(want["n_bg"], want["n_fg"], want["n_neg"]) > 0
    losses, g_e, g_d, e2, d2 = al.loss_step(m, x, label)
    with g_e, g_d, e2, d2:
        assert losses == want  # to the bits
        assert np.array_equal(g_e.to_host(), we) and np.array_equal(g_d.to_host(), wd)
        assert np.array_equal(e2.to_host(), e_host) and np.array_equal(d2.to_host(), d_host)
    l3, n_e, n_d, e3, d3 = al.loss_step(m, x, label, want_grad=False)
    with e3, d3:
        assert l3 == want and n_e is None and n_d is None
    with pytest.raises(ValueError):
        al.loss_step(m, x, label[:1])
    with pytest.raises(ValueError):  # the model keeps a context of its own
        irn_train.AffinityLoss(PathIndex(5), ctx=ctx).loss_step(m, x, label)


def test_new_symbols_are_exported(built):
    declared = _lib.check_exports()
    lib = _lib.load()
    for name in ("wsc_irn_aff_loss", "wsc_net_forward_edge_raw", "wsc_net_edge_size"):
        assert name in declared and hasattr(lib, name)
    assert _lib.IRN_LOSS_SLOTS == ref.KEYS
