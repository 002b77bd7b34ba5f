"""Oracle of the dropout sites of the 01_train training graph (nn.Dropout(p=0.5) of common_cnn.make_layers: the `D` entries of
VGG16's layer5, net/vgg16.py:44, and of M7's classifier branch, net/m7.py:41) under the project's own counter-based contract
(include/wsscam.h): tests/cls_grad_ref.py's torch passes with explicit mask multiplication at the sites, the
masks tests/seg_dropout_ref.py's numpy Philox.

Sites are numbered by the order of the `D` entries: VGG16 site 0 behind layer5's first entry and site 1 behind its second; M7 site 0
behind the layer3_p2 pool of the classifier branch, in front of the global max (which the loss head takes: the `feat` of a dropping
M7 pass is the pooled, dropped map).  On a BatchNorm net the site drops the BatchNorm's output ("<key>.bn"), on a net without it the
post-ReLU output ("<key>").  At drop_prob = 0 nothing is dropped and M7's feat is the un-pooled map, as without dropout.

The backward definition stays the chain rule EVALUATED AT THE TAPE (tests/cls_grad_ref.py).  At a BatchNorm site the mask comes from
keep_mask -- a kept BatchNorm output may be negative or exactly 0.0, so the tape cannot give it back; at a post-ReLU site it is
scale (T > 0), as behind fc6 / fc7."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import cls_grad_ref as gref
from tests.cls_grad_ref import _nchw, _nhwc, _params, _pc, _pool, _t, bn_grad_t, bn_stats_t, stack_ops
from tests.seg_dropout_ref import dropout_f32, keep_mask, philox4x32_10, scale_of  # noqa: F401  (re-exported for the tests)

# (root, batchnorm, pools, (H, W)) at B = 2 and the real widths: both stacks with and without BatchNorm, both pool families
DROP_CASES = [("vgg16", True, None, (33, 33)), ("vgg16", False, None, (40, 24)), ("m7", True, None, (40, 24)),
              ("m7", False, gref.KERAS_POOLS, (33, 33))]
DROP = (0.5, 7, 3)  # (drop_prob, seed, step) of the whole-pass tests
M7_SITE = 0

# The worst per-tensor max|g32 - g64| / max|g64| of chain_grads_drop in float32 against chain_grads_drop in float64 on ONE float32
# tape of forward_tape_drop, over DROP_CASES at DROP (drop_prob = 0.5) with dfeat = cls_grad_ref.case_dfeat: measured by
# tests/test_cls_dropout_oracle.py::test_float32_chain_error, which holds the re-measured figure to 1.5 x this.  The device's
# end-to-end bound is 64 x this (tests/test_gpu_cls_dropout.py).  The worst tensor is vgg16.layer1.3.bias of ("vgg16", True, None,
# (33, 33)); per case, in DROP_CASES order, 2.50e-6, 8.47e-7, 1.27e-6, 6.92e-7.
# The device's own worst ratios against chain_grads_drop(float64) on its tape, first measured on an MI355X, in DROP_CASES order:
# WSC_PREC_F32 4.09e-6 (vgg16.layer2.3.bias), 3.34e-6, 2.08e-6, 1.25e-6; f16x3 4.18e-6 (vgg16.layer2.2.bias), 3.34e-6, 1.71e-6,
# 1.25e-6; M7 with a strongly negative beta on one channel (the dropped zero wins the global max) 1.99e-6.  The bound
# 64 x 2.50e-6 = 1.60e-4 is there for the wiring: one wrong mask bit or pool decision is 1e-2.
R32_CHAIN_CLS_DROP = 2.50e-6


def drop_sites(root, sd):
    """{tape name of the conv a `D` entry follows: site}, by the order of the `D` entries of the stack's table"""
    sites, n, last = {}, 0, None
    for lname, layer in gref.CFG[root]:
        idx = 0
        for v in layer:
            if v == "M":
                idx, last = idx + 1, None
            elif v == "D":
                if last is not None:
                    sites[last] = n
                n, idx = n + 1, idx + 1
            else:
                last = "%s.%s.%d" % (root, lname, idx)
                idx += 3 if "%s.%s.%d.running_mean" % (root, lname, idx + 2) in sd else 2
    return sites


def mask_t(shape_nhwc, drop, site, dtype):
    """the NCHW tensor keep * scale of a site's [B][h][w][C] tensor (element index = the linear NHWC index)"""
    m = keep_mask(tuple(shape_nhwc), drop[0], drop[1], drop[2], site)
    return _nchw(m.astype(np.float64) * float(scale_of(drop[0])), dtype)


def _nhwc_shape(t):
    return (t.shape[0], t.shape[2], t.shape[3], t.shape[1])


def head_pool_t(t, pools):
    """M7's layer3_p2: MaxPool2d(2, 2), or the third row of a Keras session's pools"""
    return _pool(t, pools, 2)


def m7_head_t(t, pools, drop):
    """layer3_p1's output (NCHW) -> the map the global max reduces: pool -> mask"""
    p = head_pool_t(t, pools)
    return p * mask_t(_nhwc_shape(p), drop, M7_SITE, t.dtype)


def _forward_drop(root, P, sd, t, pools, drop, tape=None):
    """cls_grad_ref._forward with the sites active (drop[0] > 0); -> feat"""
    def keep(name, v):
        if tape is not None:
            tape[name] = v
        return v

    if not drop[0] > 0:
        return gref._forward(root, P, sd, t, pools, tape)
    sites = drop_sites(root, sd)
    keep("input", t)
    n_pool = 0
    for kind, name, bn in stack_ops(root, sd):
        if kind == "pool":
            t = keep(name, _pool(t, pools, n_pool))
            n_pool += 1
            continue
        t = F.relu(F.conv2d(t, P[name + ".weight"], P[name + ".bias"], padding=1))
        if not bn:
            if name in sites:
                t = t * mask_t(_nhwc_shape(t), drop, sites[name], t.dtype)
            keep(name, t)
            continue
        keep(name, t)
        mean, rstd = bn_stats_t(t)
        keep(name + ".stats", torch.stack([mean, rstd], 1))
        t = (t - _pc(mean)) * _pc(rstd) * _pc(P[bn + ".weight"]) + _pc(P[bn + ".bias"])
        if name in sites:
            t = t * mask_t(_nhwc_shape(t), drop, sites[name], t.dtype)
        keep(name + ".bn", t)
    return m7_head_t(t, pools, drop) if root == "m7" else t


def forward_tape_drop(root, sd, x, pools, drop, dtype=torch.float64):
    """cls_grad_ref.forward_tape with dropout: the sites' entries are the dropped, scaled values; M7's feat the pooled, dropped map"""
    tape = {}
    with torch.no_grad():
        feat = _forward_drop(root, _params(root, sd, dtype, False), sd, _t(x, dtype), pools, drop, tape)
    return gref._tape_out(tape), _nhwc(feat)


def autograd_grads_drop(root, sd, x, dfeat, pools, drop, dtype=torch.float64):
    """plain autograd of the whole training forward pass with explicit mask multiplication, d loss / d feat = dfeat NHWC"""
    P = _params(root, sd, dtype, True)
    _forward_drop(root, P, sd, _t(x, dtype), pools, drop).backward(_nchw(dfeat, dtype))
    return {n: p.grad.numpy().copy() for n, p in P.items()}


def m7_head_grad_t(x, g, pools, drop):
    """the gradient of m7_head_t at the kept input x (NCHW) for g of the pooled shape: the site's mask, then the pool's own autograd"""
    xx = x.detach().requires_grad_(True)
    head_pool_t(xx, pools).backward(g * mask_t(_nhwc_shape(g), drop, M7_SITE, g.dtype))
    return xx.grad


def chain_grads_drop(root, sd, tape, dfeat, pools, drop, dtype=torch.float64):
    """cls_grad_ref.chain_grads on a tape of a dropout forward pass, drop = (drop_prob, seed, step).  A BatchNorm site multiplies the
    incoming gradient by keep_mask * scale before the BatchNorm's backward (nothing is read off the tape for it); a post-ReLU site
    forms dz = g * scale * (T > 0).  M7: dfeat has the pooled shape and goes through the site and layer3_p2 first."""
    if not drop[0] > 0:
        return gref.chain_grads(root, sd, tape, dfeat, pools, dtype)
    P = _params(root, sd, dtype, False)
    T = {k: (_t(v, dtype) if k.endswith(".stats") else _nchw(v, dtype)) for k, v in tape.items()}
    ops = stack_ops(root, sd)
    sites = drop_sites(root, sd)
    s = float(scale_of(drop[0]))
    out_name = ["%s.bn" % name if bn else name for _, name, bn in ops]
    pool_of = {name: i for i, name in enumerate(n for k, n, _ in ops if k == "pool")}
    g = _nchw(dfeat, dtype)
    if root == "m7":
        g = m7_head_grad_t(T[out_name[-1]], g, pools, drop)
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
        relu_scale = 1.0
        if bn:
            if name in sites:
                g = g * mask_t(_nhwc_shape(g), drop, sites[name], dtype)
            st = T[name + ".stats"]
            g, dgamma, dbeta = bn_grad_t(a, st[:, 0], st[:, 1], P[bn + ".weight"], g)
            out[bn + ".weight"], out[bn + ".bias"] = dgamma.numpy().copy(), dbeta.numpy().copy()
        elif name in sites:
            relu_scale = s
        dz = g * relu_scale * (a > 0).to(dtype)
        xx = x.detach().requires_grad_(i > 0)
        w, b = P[name + ".weight"].detach().requires_grad_(True), P[name + ".bias"].detach().requires_grad_(True)
        F.conv2d(xx, w, b, padding=1).backward(dz)
        out[name + ".weight"], out[name + ".bias"] = w.grad.numpy().copy(), b.grad.numpy().copy()
        g = xx.grad if i > 0 else None
    return out
