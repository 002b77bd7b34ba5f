"""CPU: the reference of the update half of a 01_train step (tests/cls_sgd_ref.py) and the host side of the feature
(cls_train.step_lr / cyclic_lr, _lib.ClsGrad.flat_params) against independent statements.

The float64 bound of the torch comparison, from the operation count.  One step of either form is at most 6 floating-point operations
per element (Keras: lr g, mu m, their difference, mu v, two sums; torch: mu buf, + g, mu buf again, + g, lr times it, p minus it), each
with a relative rounding error of at most u64 = 2^-53 on a quantity that S = max|p0| + K lr (1 + mu) max|g| / (1 - mu) bounds (the
start plus everything K steps can move; the momentum buffer's geometric sum is below max|g| / (1 - mu)).  Errors of earlier steps are
carried with factors <= 1 + mu.  Two forms, K = 3 steps: |keras64 - torch64| <= 2 * K * 6 * (1 + mu)^K * u64 * S.
The float32 restatement against its own float64 form: the same count with u32 = 2^-24, one form: K * 6 * (1 + mu)^K * u32 * S."""
import math

import numpy as np
import torch

from oracle import cnn_ref
from tests import cls_grad_ref as gref
from tests import cls_sgd_ref as ref
from wsscam import _lib, cls_train

U64, U32 = 2.0 ** -53, 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_keras_nesterov_is_torch_nesterov_at_a_constant_rate():
    rng = np.random.default_rng(5)
    n, K, lr, mu = 4096, 3, 0.01, 0.9
    p0 = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(K)]
    S = np.abs(p0).max() + K * lr * (1 + mu) * max(np.abs(g).max() for g in gs) / (1 - mu)
    for nesterov in (True, False):
        tp = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
        opt = torch.optim.SGD([tp], lr=lr, momentum=mu, dampening=0, nesterov=nesterov)
        p64, m64 = p0.astype(np.float64), np.zeros(n)
        p32, m32 = p0, np.zeros(n, np.float32)
        for g in gs:
            tp.grad = torch.from_numpy(g.astype(np.float64))
            opt.step()
            p64, m64 = ref.sgd_step64(p64, g, m64, lr, mu, nesterov)
            # (the float32 form takes the float32 roundings of lr and mu as its scalars; so does its float64 twin below)
            p32, m32 = ref.sgd_step32(p32, g, m32, lr, mu, nesterov)
        e_torch = np.abs(p64 - tp.detach().numpy()).max()
        b_torch = 2 * K * 6 * (1 + mu) ** K * U64 * S
        # Keras' v = mu m - lr g is torch's -lr buf: the momentum slot itself
        buf = opt.state[tp]["momentum_buffer"].numpy()
        e_buf = np.abs(m64 + lr * buf).max()
        q64, w64 = p0.astype(np.float64), np.zeros(n)
        for g in gs:
            q64, w64 = ref.sgd_step64(q64, g, w64, float(np.float32(lr)), float(np.float32(mu)), nesterov)
        e_32 = np.abs(p32.astype(np.float64) - q64).max()
        b_32 = K * 6 * (1 + mu) ** K * U32 * S
        print("nesterov=%s: |keras64 - torch64| %.3e (bound %.3e), |-lr buf - v| %.3e, |keras32 - keras64| %.3e (bound %.3e)"
              % (nesterov, e_torch, b_torch, e_buf, e_32, b_32))
        assert e_torch <= b_torch and e_buf <= b_torch and e_32 <= b_32
        assert np.abs(p64 - p0).max() > 100 * b_32  # the steps moved the parameters by far more than either bound


def test_hand_computed_two_steps():
    """every value a dyadic rational: exact in float32, worked by hand.  lr = 1/4, momentum = 1/2, p = 1, m = 0, g = 2 then 1:
      nesterov   step 1: lr g = 1/2, v = 0 - 1/2 = -1/2, p = (1 + 1/2 * -1/2) - 1/2 = 1/4
                 step 2: lr g = 1/4, v = 1/2 * -1/2 - 1/4 = -1/2, p = (1/4 + 1/2 * -1/2) - 1/4 = -1/4
      plain      step 1: v = -1/2, p = 1 - 1/2 = 1/2;  step 2: v = -1/4 - 1/4 = -1/2, p = 0"""
    for nesterov, want in ((True, [(0.25, -0.5), (-0.25, -0.5)]), (False, [(0.5, -0.5), (0.0, -0.5)])):
        p, m = np.array([1.0], np.float32), np.array([0.0], np.float32)
        for g, (wp, wm) in zip((2.0, 1.0), want):
            p, m = ref.sgd_step32(p, np.array([g], np.float32), m, 0.25, 0.5, nesterov)
            assert p.dtype == np.float32 and m.dtype == np.float32 and p[0] == wp and m[0] == wm, (nesterov, g, p, m)


def test_every_operation_is_one_float32_rounding():
    """the restatement is not "float64, rounded at the end": on random data the two differ in many elements, which is what makes the
    device's bit comparison against it a test of the association and of the absence of fused operations"""
    rng = np.random.default_rng(6)
    p, g, m = (rng.standard_normal(1 << 14).astype(np.float32) for _ in range(3))
    lr, mu = np.float32(0.01), np.float32(0.9)
    p32, m32 = ref.sgd_step32(p, g, m, lr, mu)
    p64, m64 = ref.sgd_step64(p, g, m, float(lr), float(mu))
    assert (_bits(p32) != _bits(p64.astype(np.float32))).mean() > 0.05 and (_bits(m32) != _bits(m64.astype(np.float32))).mean() > 0.05
    # a NaN gradient stays in its element; -0.0 and denormals are ordinary values
    g2 = g.copy()
    g2[7] = np.nan
    pn, mn = ref.sgd_step32(p, g2, m, lr, mu)
    assert np.isnan(pn[7]) and np.isnan(mn[7]) and np.array_equal(_bits(np.delete(pn, 7)), _bits(np.delete(p32, 7)))


def test_step_lr_is_demo_py_113():
    """base_lr * droprate ** ((epoch + latest_epoch) // dropstep) at base 1e-3, droprate 0.5, dropstep 20: the exponent by hand"""
    for latest, exps in ((0, {0: 0, 19: 0, 20: 1, 79: 3}), (20, {0: 1, 19: 1, 20: 2, 79: 4})):
        for epoch, k in exps.items():
            got = cls_train.step_lr(epoch, latest)
            assert isinstance(got, np.float32) and got == np.float32(1e-3 * 0.5 ** k), (epoch, latest, got)
    assert cls_train.step_lr(45, 0, base_lr=0.02, droprate=0.1, dropstep=15) == np.float32(0.02 * 0.1 ** 3)


def test_cyclic_lr_triangle():
    base, top, step = 1e-3, 2e-2, 250
    at = lambda it: cls_train.cyclic_lr(it, base, top, step)  # noqa: E731
    assert at(0) == np.float32(base) and at(step) == np.float32(top) and at(2 * step) == np.float32(base) and at(3 * step) == np.float32(top)
    assert at(step // 2) == np.float32((base + top) / 2) and at(step + step // 2) == np.float32((base + top) / 2)  # mid-slope, up and down
    assert at(50) == np.float32(base + (top - base) * 0.2) and at(2 * step + 50) == at(50)  # the cycle repeats
    assert isinstance(at(7), np.float32) and all(at(i) < at(i + 1) for i in range(0, step - 1, 17))
    assert cls_train.cyclic_session_rates(0, base, top) == (base, top) and cls_train.cyclic_session_rates(2, base, top) == (base / 4, top / 4)


THIN = {"vgg16": [(n, [v if isinstance(v, str) else max(v // 16, 4) for v in layer]) for n, layer in cnn_ref.VGG16_CFG],
        "m7": [(n, [v if isinstance(v, str) else max(v // 16, 4) for v in layer]) for n, layer in cnn_ref.M7_CFG]}


def _fake_grad(sd, root, C):
    """a ClsGrad without a device: the layout query answered from the reference's statement of the layout"""
    g = _lib.ClsGrad.__new__(_lib.ClsGrad)
    ent, n, _ = ref.layout(sd, root, C)
    lay = []
    for name, at, lies in ent:
        conv, linear = len(lies) == 4, len(lies) == 2
        lay.append({"name": name, "conv": conv, "linear": linear, "offset": at, "size": int(np.prod(lies)),
                    "shape": (lies[3], lies[2], 3, 3) if conv else lies})
    g._param_layout, g._param_elems, g.h = lay, n, None
    return g


def test_flat_params_layout():
    for root, bn, with_bias, C in (("vgg16", True, True, 20), ("vgg16", False, False, 5), ("m7", True, False, 20), ("m7", False, True, 5)):
        sd = {k: v.numpy() for k, v in cnn_ref.make_plain_state_dict(root, THIN[root], 20, bn, seed=3).items()}
        if not with_bias:
            del sd[root + ".classifier.0.bias"]
        ent, n, grad_elems = ref.layout(sd, root, C)
        names = [e[0] for e in ent]
        # the gradient layout in front, unchanged; the Linear behind it, then its bias; no gaps
        assert names[:len(gref.param_names(root, sd))] == gref.param_names(root, sd)
        assert names[len(gref.param_names(root, sd)):] == [root + ".classifier.0.weight"] + ([root + ".classifier.0.bias"] if with_bias else [])
        assert all(ent[i][1] + int(np.prod(ent[i][2])) == (ent[i + 1][1] if i + 1 < len(ent) else n) for i in range(len(ent)))
        assert ent[len(gref.param_names(root, sd))][1] == grad_elems and grad_elems % 4 == 0
        flat = _fake_grad(sd, root, C).flat_params(sd)
        assert flat.dtype == np.float32 and np.array_equal(_bits(flat), _bits(ref.flat_params(sd, root, C)))
        # element by element, from the definition: a conv weight lies as [3][3][Cin][Cout], the Linear as [C][F]
        rng = np.random.default_rng(1)
        for name, at, lies in ent:
            v = sd[name]
            for _ in range(16):
                if v.ndim == 4:
                    co, ci, r, s = (int(rng.integers(d)) for d in v.shape)
                    assert flat[at + ((r * 3 + s) * v.shape[1] + ci) * v.shape[0] + co] == v[co, ci, r, s]
                elif v.ndim == 2:
                    c, f = int(rng.integers(C)), int(rng.integers(v.shape[1]))
                    assert flat[at + c * v.shape[1] + f] == v[c, f]
                else:
                    c = int(rng.integers(lies[0]))
                    assert flat[at + c] == v[c]
        back = ref.unflatten(flat, sd, root, C)
        assert all(np.array_equal(back[k], sd[k][:C] if ".classifier." in k else sd[k]) for k in back)
        bad = dict(sd)
        del bad[names[3]]
        try:
            _fake_grad(sd, root, C).flat_params(bad)
            raise AssertionError("a missing tensor went through")
        except ValueError:
            pass


def test_fold_is_fold_bn():
    """sc = gamma / sqrt(var + eps), b = beta - mean sc with Python floats (IEEE doubles, math.sqrt correctly rounded), each rounded
    to float once -- channel by channel, the dead cases included"""
    rng = np.random.default_rng(2)
    C = 64
    gamma, beta, mean = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
    var = rng.uniform(0.0, 2.0, C).astype(np.float32)
    var[0], gamma[1], var[2], mean[3] = 0.0, 0.0, 1e-30, 3e4
    for eps in (1e-3, float(np.float32(1e-3)), 1e-5):
        s2, b2 = ref.fold(gamma, beta, mean, var, eps)
        assert s2.dtype == np.float32 and b2.dtype == np.float32
        for c in range(C):
            sc = float(gamma[c]) / math.sqrt(float(var[c]) + eps)
            assert s2[c] == np.float32(sc) and b2[c] == np.float32(float(beta[c]) - float(mean[c]) * sc), (c, eps)
        assert s2[1] == 0 and b2[1] == beta[1] and s2[0] == np.float32(float(gamma[0]) / math.sqrt(eps))
    # the double constant 1e-3 and the float 1e-3f are different eps: the fold tells them apart
    assert not np.array_equal(_bits(ref.fold(gamma, beta, mean, var, 1e-3)[0]), _bits(ref.fold(gamma, beta, mean, var, float(np.float32(1e-3)))[0]))
