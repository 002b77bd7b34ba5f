"""Oracle of the 01_train backward pass through the plain stacks (VGG16 / M7 of 03b_irn/net/common_cnn.py:128-141 in training mode),
on torch CPU: conv(bias) -> ReLU -> BatchNorm(eps = 1e-3, batch statistics) per entry, the max pools between (MaxPool2d(2, 2), or the
TensorFlow rows of tests/keras_arch_ref.py), the `D` entries the identity.

The device's definition (include/wsscam.h) is the chain rule EVALUATED AT THE TAPE: a ReLU passes dy where the
kept output is > 0, a pool's decisions are recomputed from its kept input (autograd of that op alone: torch's first maximum in
row-major window order, the -inf padding never a candidate), BatchNorm's backward takes xh = (a - mean) rstd from the kept input and the
KEPT {mean, rstd} -- nothing is recomputed.  chain_grads states exactly that, one op at a time.  With a float64 tape it is whole-graph
autograd (tests/test_cls_grad_oracle.py); on a float32 tape, evaluated in float64, it is the reference every device gradient is held to.

Tape names: "input", per conv its state-dict key (the post-ReLU output), "<key>.bn" and "<key>.stats" ((C, 2) {mean, rstd}) on
BatchNorm nets, "pool:<i>".  Activations are NHWC numpy arrays, gradients come under state-dict names in torch's shapes."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn_ref
from tests import keras_arch_ref

EPS = 1e-3
CFG = {"vgg16": cnn_ref.VGG16_CFG, "m7": cnn_ref.M7_CFG}
KERAS_POOLS = ((3, 2, "same"),) * 3  # a Keras-side session's MaxPooling2D(3, strides 2, 'same'); m7: the third row is the classifier's

# (root, batchnorm, pools, (H, W)) at B = 2 and the real widths: both stacks, square 33 x 33 and 40 x 24, with and without BatchNorm,
# torch's 2 x 2 / 2 pools and the Keras rows -- every factor with both stacks
GRAD_CASES = [("vgg16", True, None, (33, 33)), ("vgg16", False, None, (40, 24)), ("vgg16", True, KERAS_POOLS, (40, 24)),
              ("m7", True, None, (40, 24)), ("m7", False, KERAS_POOLS, (33, 33)), ("m7", True, KERAS_POOLS, (33, 33))]
B = 2

# The worst per-tensor max|g32 - g64| / max|g64| of chain_grads in float32 against chain_grads in float64 on ONE float32 tape, over
# GRAD_CASES with dfeat = 1e-3 N(0, 1): measured by tests/test_cls_grad_oracle.py::test_float32_chain_error, which holds the
# re-measured figure to 1.5 x this.  The device's end-to-end bound is 64 x this (tests/test_gpu_cls_grad.py).  The worst tensor is
# vgg16.layer1.3.bias of ("vgg16", True, KERAS_POOLS, (40, 24)); per case 1.45e-6, 9.09e-7, 1.83e-6, 1.20e-6, 8.37e-7, 1.40e-6.
# The device's own worst ratios against chain_grads(float64) on its tape, first measured on an MI355X: WSC_PREC_F32 4.05e-6
# (vgg16.layer1.3.bias, VGG16 + BatchNorm at 33 x 33), f16x3 5.06e-6 (vgg16.layer4.0.weight, VGG16 + BatchNorm, Keras pools, 40 x 24);
# the M7 cases 1.6e-6 - 2.1e-6.  The bound 64 x 1.83e-6 = 1.17e-4 is there for the wiring: one wrong mask or pool decision is 1e-2.
R32_CHAIN_CLS = 1.83e-6


def case_id(case):
    root, bn, pools, hw = case
    return "%s-%s-%s-%dx%d" % (root, "bn" if bn else "nobn", "keras" if pools else "torch", hw[0], hw[1])


@functools.lru_cache(maxsize=None)
def state_dict(root, batchnorm):
    """the real-width weights: built once per (root, batchnorm), shared, never modified"""
    return cnn_ref.make_plain_state_dict(root, CFG[root], 20, batchnorm, seed=21 if root == "vgg16" else 22)


def net_input(hw):
    return np.random.default_rng(700 + hw[0] + 3 * hw[1]).normal(0, 1, (B, 3, hw[0], hw[1])).astype(np.float32)


def case_dfeat(case, shape):
    root, bn, pools, hw = case
    rng = np.random.default_rng(2300 + hw[1] + 5 * bool(bn) + 11 * bool(pools) + (1 if root == "m7" else 0))
    return (1e-3 * rng.standard_normal(shape)).astype(np.float32)


def stack_ops(root, sd):
    """[(kind, tape name, BatchNorm key or None)] in execution order: ('conv', '<key>', bn) / ('pool', 'pool:<i>', None)"""
    ops, n_pool = [], 0
    for lname, layer in CFG[root]:
        idx = 0
        for v in layer:
            if v == "M":
                ops.append(("pool", "pool:%d" % n_pool, None))
                n_pool, idx = n_pool + 1, idx + 1
            elif v == "D":
                idx += 1
            else:
                key, bn = "%s.%s.%d" % (root, lname, idx), "%s.%s.%d" % (root, lname, idx + 2)
                has_bn = bn + ".running_mean" in sd
                ops.append(("conv", key, bn if has_bn else None))
                idx += 3 if has_bn else 2
    return ops


def param_names(root, sd):
    """the layout's names: net.common.plain_module_order without the classifier's Linear"""
    out = []
    for kind, key, bn in stack_ops(root, sd):
        if kind == "conv":
            out += [key + ".weight", key + ".bias"] + ([bn + ".weight", bn + ".bias"] if bn else [])
    return out


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def _nchw(a, dtype):
    return _t(a, dtype).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _pool(t, pools, i):
    if pools is None:
        return F.max_pool2d(t, 2, 2)
    k, stride, padding = pools[i]
    return keras_arch_ref.tf_max_pool_t(t, int(k), int(stride), padding == "same")


def _pc(v):
    return v[None, :, None, None]


def bn_stats_t(a, eps=EPS):
    """NCHW -> (mean, rstd) per channel: the population variance, two passes"""
    mean = a.mean(dim=(0, 2, 3))
    var = ((a - _pc(mean)) ** 2).mean(dim=(0, 2, 3))
    return mean, 1.0 / torch.sqrt(var + eps)


def _forward(root, P, sd, t, pools, tape=None):
    """the training-mode forward pass on tensors; tape: a dict that receives every kept tensor (NCHW; '.stats' as (C, 2))"""
    def keep(name, v):
        if tape is not None:
            tape[name] = v
        return v

    keep("input", t)
    n_pool = 0
    for kind, name, bn in stack_ops(root, sd):
        if kind == "pool":
            t = keep(name, _pool(t, pools, n_pool))
            n_pool += 1
            continue
        t = keep(name, F.relu(F.conv2d(t, P[name + ".weight"], P[name + ".bias"], padding=1)))
        if bn:
            mean, rstd = bn_stats_t(t)
            keep(name + ".stats", torch.stack([mean, rstd], 1))
            t = keep(name + ".bn", (t - _pc(mean)) * _pc(rstd) * _pc(P[bn + ".weight"]) + _pc(P[bn + ".bias"]))
    return t


def _params(root, sd, dtype, requires_grad):
    return {n: sd[n].detach().to(dtype).clone().requires_grad_(requires_grad) for n in param_names(root, sd)}


def _tape_out(tape):
    return {k: (v.detach().numpy() if k.endswith(".stats") else _nhwc(v)) for k, v in tape.items()}


def forward_tape(root, sd, x, pools, dtype=torch.float64):
    """x (B, 3, H, W) -> ({tape name: NHWC array of `dtype`}, feat NHWC): the training forward pass in `dtype`, everything kept"""
    tape = {}
    with torch.no_grad():
        feat = _forward(root, _params(root, sd, dtype, False), sd, _t(x, dtype), pools, tape)
    return _tape_out(tape), _nhwc(feat)


def autograd_grads(root, sd, x, dfeat, pools, dtype=torch.float64):
    """{state-dict name: gradient in torch's shape}: plain autograd of the whole training forward pass, d loss / d feat = dfeat NHWC"""
    P = _params(root, sd, dtype, True)
    _forward(root, P, sd, _t(x, dtype), pools).backward(_nchw(dfeat, dtype))
    return {n: p.grad.numpy().copy() for n, p in P.items()}


def bn_grad_t(a, mean, rstd, gamma, dy):
    """(da, dgamma, dbeta) of training-mode BatchNorm at the KEPT statistics (NCHW tensors, per-channel vectors)"""
    M = a.shape[0] * a.shape[2] * a.shape[3]
    xh = (a - _pc(mean)) * _pc(rstd)
    dbeta, dgamma = dy.sum(dim=(0, 2, 3)), (dy * xh).sum(dim=(0, 2, 3))
    return _pc(gamma * rstd) * (dy - _pc(dbeta) / M - xh * _pc(dgamma) / M), dgamma, dbeta


def chain_grads(root, sd, tape, dfeat, pools, dtype=torch.float64):
    """The chain rule evaluated at `tape` ({name: NHWC array; '.stats' (C, 2)}, e.g. the device's own), in `dtype`: per op, autograd
    of that one op on its kept input (conv, pool), the ReLU mask from its kept output, BatchNorm from its kept input and kept
    statistics.  -> {state-dict name: gradient in torch's shape}, numpy arrays of `dtype`."""
    P = _params(root, sd, dtype, False)
    T = {k: (_t(v, dtype) if k.endswith(".stats") else _nchw(v, dtype)) for k, v in tape.items()}
    ops = stack_ops(root, sd)
    out_name = ["%s.bn" % name if bn else name for _, name, bn in ops]  # the entry the next op read
    pool_of = {name: i for i, name in enumerate(n for k, n, _ in ops if k == "pool")}
    g = _nchw(dfeat, dtype)
    out = {}
    for i in range(len(ops) - 1, -1, -1):
        kind, name, bn = ops[i]
        x = T[out_name[i - 1] if i > 0 else "input"]
        if kind == "pool":
            xx = x.detach().requires_grad_(True)
            _pool(xx, pools, pool_of[name]).backward(g)
            g = xx.grad
            continue
        a = T[name]
        if bn:
            st = T[name + ".stats"]
            g, dgamma, dbeta = bn_grad_t(a, st[:, 0], st[:, 1], P[bn + ".weight"], g)
            out[bn + ".weight"], out[bn + ".bias"] = dgamma.numpy().copy(), dbeta.numpy().copy()
        dz = g * (a > 0).to(dtype)
        xx = x.detach().requires_grad_(i > 0)
        w, b = P[name + ".weight"].detach().requires_grad_(True), P[name + ".bias"].detach().requires_grad_(True)
        F.conv2d(xx, w, b, padding=1).backward(dz)
        out[name + ".weight"], out[name + ".bias"] = w.grad.numpy().copy(), b.grad.numpy().copy()
        g = xx.grad if i > 0 else None
    return out


def worst_ratio(got, ref):
    """(worst max|got - ref| / max|ref| over the tensors, its name)"""
    worst = (0.0, "")
    for n, r in ref.items():
        r = np.asarray(r, np.float64)
        worst = max(worst, (float(np.abs(np.asarray(got[n], np.float64) - r).max() / np.abs(r).max()), n))
    return worst


# ---- float64 statements of the two BatchNorm entries on given float32 operands, each with the quantities its error bound needs --
def bn_train_ref(a, gamma, beta, eps=EPS):
    """a (M, C) float32 -> float64 (mean, var, rstd, y): two passes"""
    a = np.asarray(a, np.float64)
    mean = a.mean(0)
    var = ((a - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + eps)
    return mean, var, rstd, (a - mean) * rstd * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def bn_grad_ref(a, stats, gamma, dy):
    """a, dy (M, C) float32, stats (C, 2) the float32 {mean, rstd} of the forward pass -> float64 (da, dgamma, dbeta, xh)"""
    a, dy, g = np.asarray(a, np.float64), np.asarray(dy, np.float64), np.asarray(gamma, np.float64)
    mean, rstd = np.asarray(stats[:, 0], np.float64), np.asarray(stats[:, 1], np.float64)
    xh = (a - mean) * rstd
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    M = a.shape[0]
    return g * rstd * (dy - dbeta / M - xh * dgamma / M), dgamma, dbeta, xh


def pool_grad_ref(x, dy, pool):
    """x (N, H, W, C), dy the pool's output size, pool ('tf', k, stride, same) or ('torch', k, stride, pad) -> float64 dx: torch's
    max-pool autograd on the -inf padded input"""
    f64 = torch.float64
    xx = _nchw(x, f64).requires_grad_(True)
    kind, k, stride, last = pool
    y = keras_arch_ref.tf_max_pool_t(xx, k, stride, bool(last)) if kind == "tf" else F.max_pool2d(xx, k, stride, last)
    assert tuple(y.shape) == tuple(_nchw(dy, f64).shape), (tuple(y.shape), np.shape(dy))
    y.backward(_nchw(dy, f64))
    return _nhwc(xx.grad)


def pool_out_hw(H, W, pool):
    kind, k, stride, last = pool
    if kind == "tf":
        return keras_arch_ref.tf_pool_axis(H, k, stride, bool(last))[0], keras_arch_ref.tf_pool_axis(W, k, stride, bool(last))[0]
    return (H + 2 * last - k) // stride + 1, (W + 2 * last - k) // stride + 1
