"""GPU: the backward pass of the IRNet heads (csrc/irn_grad.hip, wsc_net_backward_edge; EdgeDisplacement.backward_dev,
irn_train.AffinityLoss.grad_step) against the float64 oracle tests/irn_grad_ref.py.

Bounds (each test prints the figure it asserts on):
  ReLU mask + upsample adjoint  elementwise |d| <= (n + 2) u sum|terms|, u = 2^-24, n the element's number of terms: the weights
               (multiples of 1 / 8) and their products are exact, every term costs the one rounding of its fmaf; the bound holds
               for any order.  With small-integer gradients the result is float64's exactly.
  GroupNorm backward  max|d| <= 8 R32_GN max|g64| per output: the device works in double from the forward's float32
               statistics, so its error lies below the float32 evaluation's own (R32_GN, irn_grad_ref.py); 8 covers the float
               rounding of mean / rstd and the output rounding.
  tape         edge / dp bit for bit those of forward_edge_raw; every entry within 2e-4 max(1, max|want|) of the float64 op on the
               entries it read (the tolerance of tests/test_gpu_irn.py); statistics: one float rounding of the float64 value.
  end to end   per parameter max|d| <= 64 R32_IRN_CHAIN max|g64| against head_grads (float64) on the device's own tape: the
               margin wsc_net_backward_seg was given.  It guards wiring (a wrong slice, crop, mask, transpose or head order is
               an O(1e-2) error); the arithmetic is held by the per-op bounds.
Every device output has GUARD floats of CANARY behind it that must survive, must be overwritten entirely, and every op is called
twice and must repeat its bits."""
import functools

import numpy as np
import pytest

from oracle import cnn_ref, irn_ref
from tests import irn_grad_ref as gref
from tests import irn_loss_ref
from tests.test_gpu_irn_loss import thin_net
from wsscam import _lib, irn_train
from wsscam.misc.indexing import PathIndex
from wsscam.net import resnet50_irn
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

CANARY = np.float32(-777.25)
GUARD = 256  # floats of CANARY behind every device output
U = 2.0 ** -24


def _canary(ctx, shape):
    return DeviceMaps.from_host(ctx, np.full((int(np.prod(shape)) + GUARD,), CANARY, np.float32))


def _guarded(ctx, a):
    """a host array on the device with GUARD canaries behind it (an input the call must not run past either)"""
    return DeviceMaps.from_host(ctx, np.concatenate([np.ascontiguousarray(a, np.float32).ravel(), np.full((GUARD,), CANARY, np.float32)]))


def _checked(buf, shape, what):
    flat = buf.to_host().ravel()
    n = int(np.prod(shape))
    assert flat.size == n + GUARD
    assert np.array_equal(flat[n:].view(np.uint32), np.full((GUARD,), CANARY, np.float32).view(np.uint32)), what + ": a store behind the output"
    assert not (flat[:n] == CANARY).any(), what + ": an element was not written"
    return flat[:n].reshape(shape).copy()


def _relu_like(rng, shape):
    """post-ReLU-like: half zeros, the positives multiples of 1/4"""
    return (np.maximum(rng.integers(-8, 9, shape), 0) / 4.0).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- ReLU mask + upsample adjoint ------------------------------------------------------------------------------------------------
# (N, H, W, C, up, Hd, Wd, Ctot, coff); the last one reaches the scalar form (C, coff no multiples of 4)
UP_CASES = [(2, 9, 9, 32, 2, 17, 17, 192, 64), (1, 5, 5, 32, 4, 17, 17, 192, 128), (2, 5, 5, 256, 2, 9, 9, 768, 512),
            (1, 1, 1, 32, 4, 3, 2, 192, 96), (1, 1, 7, 64, 2, 2, 14, 448, 0), (3, 6, 4, 64, 1, 6, 4, 448, 0),
            (2, 8, 8, 256, 2, 16, 16, 448, 192), (2, 5, 5, 30, 2, 9, 9, 101, 7)]
UP_RUNS = [(c, "relu", False) for c in UP_CASES] + [(c, "relu", True) for c in UP_CASES] + \
          [(UP_CASES[0], "negative", False), (UP_CASES[0], "positive", False), (UP_CASES[7], "negative", False)]


def _up_run(ctx, case, dcat, cat):
    N, H, W, C, up, Hd, Wd, Ctot, coff = case
    with _guarded(ctx, dcat) as d, _guarded(ctx, cat) as c, _canary(ctx, (N, H, W, C)) as out:
        _lib.relu_upsample_grad_nhwc(ctx, d.ptr, c.ptr, N, H, W, C, up, Hd, Wd, Ctot, coff, out.ptr)
        return _checked(out, (N, H, W, C), "dy")


@pytest.mark.parametrize("case,fill,integer", UP_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_relu_upsample_grad(ctx, case, fill, integer):
    N, H, W, C, up, Hd, Wd, Ctot, coff = case
    rng = np.random.default_rng(sum(case) + len(fill))
    shape = (N, Hd, Wd, Ctot)
    cat = _relu_like(rng, shape) if fill == "relu" else (-_relu_like(rng, shape) if fill == "negative" else _relu_like(rng, shape) + 0.25)
    dcat = rng.integers(-4, 5, shape).astype(np.float32) if integer else rng.standard_normal(shape).astype(np.float32)
    want, mag, terms = gref.up_relu_grad(dcat, cat, H, W, C, up, coff)
    got = _up_run(ctx, case, dcat, cat)
    again = _up_run(ctx, case, dcat, cat)
    assert np.array_equal(_bits(got), _bits(again))
    err = np.abs(got.astype(np.float64) - want)
    print("relu_upsample_grad %s %s%s: max |err| / (u sum|terms|) %.3g, most terms %d" %
          (case, fill, " integer" if integer else "", float((err / np.maximum(U * mag, 1e-300)).max()) if mag.max() > 0 else 0.0, int(terms.max())))
    if fill == "negative":
        assert np.array_equal(_bits(got), np.zeros(got.shape, np.uint32))  # exactly +0.0
    elif integer:
        assert np.array_equal(got.astype(np.float64), want)
    else:
        assert (err <= (terms + 2) * U * mag).all()
        assert np.abs(want).max() > 0


# ---- GroupNorm backward -----------------------------------------------------------------------------------------------------------
def _gn_run(ctx, case, z, dy, gamma):
    N, H, W, C, G = case
    with _guarded(ctx, z) as zd, _guarded(ctx, dy) as dd, _canary(ctx, (N, H, W, C)) as dz, _canary(ctx, (C,)) as dg, _canary(ctx, (C,)) as db:
        _lib.group_norm_grad_nhwc(ctx, zd.ptr, dd.ptr, N, H, W, C, gamma, G, gref.EPS, dz.ptr, dg.ptr, db.ptr)
        return _checked(dz, (N, H, W, C), "dz"), _checked(dg, (C,), "dgamma"), _checked(db, (C,), "dbeta")


@pytest.mark.parametrize("case", gref.GN_CASES + [gref.GN_CONSTANT_CASE, (2, 7, 5, 6, 2)], ids=str)
def test_group_norm_grad(ctx, case):
    """(the last case, C = 6, reaches the scalar form)"""
    constant = case == gref.GN_CONSTANT_CASE
    z, dy, gamma = gref.gn_case(case, 5, constant=constant)
    want = gref.group_norm_grad(z, dy, gamma, case[4])
    got = _gn_run(ctx, case, z, dy, gamma)
    again = _gn_run(ctx, case, z, dy, gamma)
    for key, g, a, w in zip(("dz", "dgamma", "dbeta"), got, again, want):
        assert np.array_equal(_bits(g), _bits(a)), key
        assert np.isfinite(g).all(), key
        top = np.abs(w).max()
        ratio = float(np.abs(g.astype(np.float64) - w).max() / top)
        print("group_norm_grad %s%s %s: max|d| / max|g64| %.3e (bound %.3e)" % (case, " constant group" if constant else "", key, ratio,
                                                                             8 * gref.R32_GN[key]))
        assert ratio <= 8 * gref.R32_GN[key], key


# ---- the nets ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resnet_sd():
    return irn_ref.make_resnet50_irn_state_dict(seed=3)


@functools.lru_cache(maxsize=None)
def model(arch, precision=None):
    """-> (EdgeDisplacement wrapper, torch state dict); one per (arch, precision) for the module"""
    if arch != "resnet50":
        m, sd, _ = thin_net(arch)
        return m, sd
    m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=64, stride=4, precision=precision)
    m.load_state_dict(resnet_sd())
    m.eval().cuda(0)
    return m, resnet_sd()


def net_input(N, S):
    return np.random.default_rng(100 + N + S).normal(0, 1, (N, 3, S, S)).astype(np.float32)


def host_tape(tape):
    return {e["name"]: tape.entry(e["name"]) for e in tape.entries}


@pytest.mark.parametrize("precision", [_lib.PREC_F16X3, _lib.PREC_F32], ids=["f16x3", "f32"])
def test_tape(precision):
    m, sd = model("resnet50", precision)
    ctx, net = m.ctx, m._ensure_net()
    N, S = 2, 68
    x = net_input(N, S)
    edge, dp = m.forward_train_dev(x)
    with edge, dp:
        want_e, want_d = edge.to_host(), dp.to_host()
    entries, elems = net.edge_tape_plan(N, S)
    (He, We), (Hd, Wd) = net.edge_size(S)
    with DeviceMaps.from_host(ctx, x) as xd, _canary(ctx, (elems,)) as tp, _canary(ctx, (N, He, We)) as e, _canary(ctx, (N, 2, Hd, Wd)) as d:
        net.forward_edge_tape(xd.ptr, N, S, tp.ptr, elems, e.ptr, d.ptr)
        got_e, got_d = _checked(e, (N, He, We), "edge"), _checked(d, (N, 2, Hd, Wd), "dp")
        flat = tp.to_host()
    assert np.array_equal(_bits(got_e), _bits(want_e)) and np.array_equal(_bits(got_d), _bits(want_d))
    assert (flat[elems:] == CANARY).all()
    tape = {}
    for en in entries:  # every entry written entirely, on a 256-byte line
        n = N * en["Ho"] * en["Wo"] * en["C"]
        assert en["offset"] % 64 == 0 and not (flat[en["offset"]:en["offset"] + n] == CANARY).any(), en["name"]
        tape[en["name"]] = flat[en["offset"]:en["offset"] + n].reshape(N, en["Ho"], en["Wo"], en["C"]).copy()
    assert [tape["x%d" % k].shape[1] for k in range(1, 6)] == [17, 17, 9, 5, 5]
    assert tape["cat0"].shape == (N, 17, 17, 192) and not tape["cat0"][..., 160:].any()  # the padding channels
    want = gref.replay(tape, sd, "resnet50")
    worst = (0.0, "")
    for name, w in want.items():
        g = tape[name].astype(np.float64)
        if name.endswith(".stats"):  # one float rounding of the float64 value from the same z
            assert (np.abs(g - w) <= 2.0 ** -23 * np.abs(w) + 1e-12).all(), name
            continue
        r = float(np.abs(g - w).max() / max(1.0, np.abs(w).max()))
        worst = max(worst, (r, name))
        assert r <= 2e-4, (name, r)
    print("tape entries vs the float64 op on the entries they read: worst %.3e at %s" % worst)
    if precision == _lib.PREC_F32:
        # the statistics are the ones wsc_group_norm_nhwc forms: that call on the taped z writes the taped concat slice
        for head, up, coff in (("fc_edge3", 2, 64), ("fc_edge2", 1, 32)):
            z = tape[head + ".z"]
            with DeviceMaps.from_host(ctx, z) as zd, DeviceMaps.from_host(ctx, np.zeros((N, 17, 17, 192), np.float32)) as y:
                _lib.group_norm_nhwc(ctx, zd.ptr, N, z.shape[1], z.shape[2], 32, sd[head + ".1.weight"].numpy(), sd[head + ".1.bias"].numpy(), 4,
                                     1e-5, up, True, 17, 17, 192, coff, _lib.PREC_F32, y.ptr)
                assert np.array_equal(_bits(y.to_host()[..., coff:coff + 32]), _bits(tape["cat0"][..., coff:coff + 32])), head


E2E = [("resnet50", 64, 2, _lib.PREC_F32), ("resnet50", 64, 2, _lib.PREC_F16X3), ("resnet50", 68, 2, _lib.PREC_F32),
       ("resnet50", 68, 2, _lib.PREC_F16X3), ("resnet50", 64, 1, _lib.PREC_F16X3), ("resnet50", 64, 3, _lib.PREC_F16X3),
       ("vgg16", 64, 2, None), ("m7", 64, 2, None)]


@pytest.mark.parametrize("arch,S,N,precision", E2E, ids=lambda v: str(v))
def test_backward_edge_vs_oracle(arch, S, N, precision):
    m, sd = model(arch, precision)
    ctx, net = m.ctx, m._ensure_net()
    x = net_input(N, S)
    edge, dp, tape = m.forward_train_dev(x, keep=True)
    with edge, dp, tape:
        rng = np.random.default_rng(S + N)
        d_edge = (1e-3 * rng.standard_normal(edge.shape)).astype(np.float32)
        d_dp = (1e-3 * rng.standard_normal(dp.shape)).astype(np.float32)
        if arch == "m7":
            assert edge.shape[1] == 2 * dp.shape[2]
        grad = m.irn_grad()
        flats = []
        with _guarded(ctx, d_edge) as de, _guarded(ctx, d_dp) as dd:
            for _ in range(2):
                with _canary(ctx, (grad.grad_elems,)) as out:
                    net.backward_edge(grad, N, S, tape.maps.ptr, tape.elems, de.ptr, dd.ptr, out.ptr)
                    flats.append(_checked(out, (grad.grad_elems,), "grad"))
            assert np.array_equal(_bits(flats[0]), _bits(flats[1]))
            g = m.backward_dev(tape, DeviceMaps(ctx, d_edge.shape, np.float32, de.buf), DeviceMaps(ctx, d_dp.shape, np.float32, dd.buf))
            with_names = g.to_state_dict()
            assert np.array_equal(_bits(g.maps.to_host()), _bits(flats[0]))
            g.maps.free()
        th = host_tape(tape)
    want = gref.head_grads(th, sd, arch, d_edge, d_dp)
    edge_names, dp_names = gref.param_names(arch)
    # exactly the head parameters of the state dict, in the order of trainable_parameters(), no entry for padding channels
    assert [e["name"] for e in grad.layout] == edge_names + dp_names and g.groups == (edge_names, dp_names)
    assert sorted(edge_names + dp_names) == sorted(k for k in sd if k.startswith("fc_"))
    assert all(with_names[n].shape == tuple(sd[n].shape) for n in with_names)
    assert grad.grad_elems == sum(int(np.prod(sd[n].shape)) for n in with_names)
    worst = gref.worst_ratio(with_names, want)
    print("backward_edge %s S = %d N = %d: worst max|d| / max|g64| %.3e at %s (bound %.3e)" % ((arch, S, N) + worst + (64 * gref.R32_IRN_CHAIN,)))
    for n, w in want.items():
        assert np.abs(w).max() > 0, n
        assert np.abs(with_names[n].astype(np.float64) - w).max() <= 64 * gref.R32_IRN_CHAIN * np.abs(w).max(), n


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_grad_step(monkeypatch):
    m, sd = model("vgg16")
    ctx = m.ctx
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, (2, 3, 64, 64)).astype(np.float32)
    label = irn_loss_ref.block_labels(rng, 2, 16, 16)
    al = irn_train.AffinityLoss(PathIndex(5), ctx=ctx)
    want_l, g_e, g_d, e, d, tape = al.loss_step(m, x, label, keep=True)
    with g_e, g_d, e, d, tape, m.backward_dev(tape, g_e, g_d) as want:
        plain = al.loss_step(m, x, label)
        with plain[1], plain[2], plain[3], plain[4]:  # keeping the tape changes no bit
            assert plain[0] == want_l and np.array_equal(_bits(plain[3].to_host()), _bits(e.to_host()))
        losses, grads = al.grad_step(m, x, label)
        with grads:
            assert losses == want_l  # to the bits
            assert np.array_equal(_bits(grads.maps.to_host()), _bits(want.maps.to_host())) and np.abs(grads.maps.to_host()).max() > 0
            one = grads.to_state_dict()["fc_dp7.0.weight"]
            assert one.shape == (256, 448, 1, 1)
            off = next(en["offset"] for en in grads.layout if en["name"] == "fc_dp7.0.weight")
            assert grads.ptr("fc_dp7.0.weight") == grads.maps.ptr + 4 * off
        # a second step: the IrnGrad object and its workspace are reused, and every buffer of the step goes back
        obj = m._irn_grad
        handed = []
        alloc0 = ctx.alloc

        def alloc(nbytes, pooled=False):
            handed.append(alloc0(nbytes, pooled=pooled))
            return handed[-1]

        monkeypatch.setattr(ctx, "alloc", alloc)
        losses2, grads2 = al.grad_step(m, x, label)
        monkeypatch.undo()
        with grads2:
            assert m._irn_grad is obj and losses2 == want_l
            assert [b.ptr for b in handed if b.ptr is not None] == [grads2.maps.ptr]
            assert np.array_equal(_bits(grads2.maps.to_host()), _bits(want.maps.to_host()))
    with pytest.raises(ValueError):
        al.grad_step(m, x, label[:1])
    other = _lib.Context(0)
    try:
        with pytest.raises(ValueError):  # the model keeps a context of its own
            irn_train.AffinityLoss(PathIndex(5), ctx=other).grad_step(m, x, label)
    finally:
        other.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(ctx):
    m, sd = model("vgg16")
    mctx, net = m.ctx, m._ensure_net()
    N, S = 2, 64
    entries, elems = net.edge_tape_plan(N, S)
    grad = m.irn_grad()
    canary = np.full((grad.grad_elems,), CANARY, np.float32)
    with DeviceMaps(mctx, (elems,), np.float32) as tape, DeviceMaps.from_host(mctx, np.zeros((N, 16, 16), np.float32)) as de, \
            DeviceMaps.from_host(mctx, np.zeros((N, 2, 16, 16), np.float32)) as dd, DeviceMaps.from_host(mctx, canary) as out, \
            DeviceMaps.from_host(mctx, net_input(N, S)) as xd, DeviceMaps.from_host(mctx, np.full((N * 16 * 16 * 3,), CANARY, np.float32)) as maps:
        for kw in ({"tape_elems": elems - 64}, {"grad_elems": grad.grad_elems - 1}):
            with pytest.raises(_lib.WscError) as ei:
                grad.backward(N, S, tape.ptr, kw.get("tape_elems", elems), de.ptr, dd.ptr, out.ptr, grad_elems=kw.get("grad_elems"))
            assert ei.value.status == _lib.WSC_ERR_INVALID
        with pytest.raises(_lib.WscError) as ei:  # a short tape in the forward pass
            net.forward_edge_tape(xd.ptr, N, S, tape.ptr, elems - 64, maps.ptr, maps.ptr + 4 * N * 256)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        with pytest.raises(_lib.WscError) as ei:  # the workspace belongs to the stream of the context the object was created on
            grad.backward(N, S, tape.ptr, elems, de.ptr, dd.ptr, out.ptr, ctx=ctx)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        mctx.sync()
        assert np.array_equal(out.to_host(), canary) and (maps.to_host() == CANARY).all()  # nothing was launched
        # mismatched gradient shapes
        et = irn_train.EdgeTape(tape, entries, N, S)
        with DeviceMaps(mctx, (N, 2, 16, 15), np.float32) as bad_d, DeviceMaps(mctx, (N, 15, 16), np.float32) as bad_e:
            for a, b in ((de, bad_d), (bad_e, dd), (de.to_host(), dd)):
                with pytest.raises(ValueError):
                    m.backward_dev(et, a, b)
        with pytest.raises(ValueError):
            m.backward_dev(tape, de, dd)
        assert np.array_equal(out.to_host(), canary)
    bad = {k: v.numpy() for k, v in sd.items()}
    bad["fc_dp6.0.weight"] = np.zeros((256, 704, 1, 1), np.float32)
    with pytest.raises(_lib.WscError) as ei:
        _lib.IrnGrad(net, bad)
    assert ei.value.status == _lib.WSC_ERR_SHAPE and "fc_dp6" in str(ei.value)
    # a CAM net has no heads, no tape and no backward pass
    cam_sd = {k: v.numpy() for k, v in cnn_ref.make_resnet50_cam_state_dict(20, seed=0).items()}
    cam = _lib.Net(ctx, _lib.ARCH_RESNET50_CAM, cam_sd, 20, _lib.PREC_F16)
    try:
        with pytest.raises(_lib.WscError) as ei:
            cam.edge_tape_plan(1, 64)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        with pytest.raises(_lib.WscError) as ei:
            _lib.IrnGrad(cam, cam_sd)
        assert ei.value.status == _lib.WSC_ERR_INVALID
    finally:
        cam.close()
