"""Oracle of the SEC / DSRG DeepLab-VGG16 backward pass (opt.compute_gradients of 03a_sec-dsrg/model.py:382-387 at drop_prob = 0),
on torch CPU, beside tests/deeplab_ref.py whose layer rules it shares.

The device's definition (include/wsscam.h) is the chain rule EVALUATED AT THE TAPE: the kept activations
are the values the next op read in the forward pass, a ReLU passes dy where the kept OUTPUT is > 0, a pool's decisions are
recomputed from its kept INPUT.  chain_grads states exactly that, one op at a time, each op's derivative by autograd of that op
alone.  With a float64 tape it is whole-graph autograd (tests/test_deeplab_grad_oracle.py); on a float32 tape, evaluated in
float64, it is the reference every device gradient is held to.

Tape names: "input", the trunk's layers, "pool:0" ... "pool:4" (behind conv1_2, conv2_2, conv3_3, conv4_3, conv5_3), "pool5a",
and every branch's "fc6[_k]", "fc7[_k]".  Activations are NHWC numpy arrays, weights HWIO, as in deeplab_ref."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.deeplab_ref import (ASPP_RATES, LFOV_RATE, THIN_CASES, TRUNK, avg_pool_same_t, layer_weights, max_pool_same_t, net_input,
                               random_weights)

# The worst per-layer max|g32 - g64| / max|g64| of chain_grads in float32 against chain_grads in float64 on ONE float32 tape, over
# GRAD_CASES at B = 2 with dfc8 = 1e-3 N(0, 1): measured by tests/test_deeplab_grad_oracle.py::test_float32_chain_error, which holds
# the re-measured figure to 1.5 x this.  The device's end-to-end bound is 64 x this (tests/test_gpu_seg_grad.py).
R32_CHAIN = 2.08e-6

GRAD_CASES = THIN_CASES + [("SEC", 5, (97, 97)), ("DSRG", 5, (97, 97))]

# The real widths (64 / 128 / 256 / 512 / 512, fc 1024, 21 classes), He-scaled like a checkpoint: (method, C, (H, W), B).  65 x 65 is
# a 9 x 9 map (SEC's fc6 and DSRG's fc6_2 ... fc6_4: the centre tap only; fc6_1 at rate 6: all nine), 64 x 48 an 8 x 6 map (fc6_1: the
# middle column of taps only).
FULL_WIDTHS = (64, 128, 256, 512, 512)
FULL_FC_WIDTH = 1024
FULL_GRAD_CASES = [("SEC", 21, (65, 65), 1), ("DSRG", 21, (65, 65), 1), ("DSRG", 21, (64, 48), 2)]

# R32_CHAIN's figure over FULL_GRAD_CASES (full_case's inputs, full_dfc8's gradient): the worst layer is conv2_1 of
# ("DSRG", 21, (65, 65), 1) (SEC 65 x 65: 1.05e-6 at conv1_2; DSRG 64 x 48, B = 2: 1.46e-6 at conv2_1); measured by
# tests/test_deeplab_grad_oracle.py::test_float32_chain_error_full_width, which holds the re-measured figure to 1.5 x this.  The
# device's full-width end-to-end bound is 64 x this.
R32_CHAIN_FULL = 1.54e-6


@functools.lru_cache(maxsize=None)
def full_weights(method, C):
    """the weights of the forward pass's full-width test: built once per (method, C), shared, never modified"""
    return random_weights(method, C, fc_width=FULL_FC_WIDTH, seed=11, widths=FULL_WIDTHS)


def full_case(case):
    """-> (weights, x) of a FULL_GRAD_CASES entry: the weights and the input recipe of the forward pass's full-width test"""
    method, C, hw, B = case
    return full_weights(method, C), net_input(B, hw[0], hw[1], 12)


def full_dfc8(case, shape):
    """d loss / d fc8 of a FULL_GRAD_CASES entry: 1e-3 N(0, 1), the seed from the case"""
    method, C, hw, B = case
    rng = np.random.default_rng(1900 + 3 * C + hw[1] + 7 * B + (1 if method == "SEC" else 0))
    return (1e-3 * rng.standard_normal(shape)).astype(np.float32)


POOL_AFTER = {"conv1_2": 2, "conv2_2": 2, "conv3_3": 2, "conv4_3": 1, "conv5_3": 1}  # layer -> stride of the max pool behind it


def branches(method):
    """[(suffix, rate)] in the order the reference sums them"""
    return [("", LFOV_RATE)] if method == "SEC" else [("_%d" % (k + 1), r) for k, r in enumerate(ASPP_RATES)]


def trunk_ops():
    """[(tape name, 'conv' | 'max' | 'avg', dilation or stride)] in execution order"""
    ops, n = [], 0
    for layer in TRUNK:
        ops.append((layer, "conv", 2 if layer.startswith("conv5") else 1))
        if layer in POOL_AFTER:
            ops.append(("pool:%d" % n, "max", POOL_AFTER[layer]))
            n += 1
    ops.append(("pool5a", "avg", 1))
    return ops


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def _nchw(a, dtype):
    return _t(a, dtype).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _conv(t, w_oihw, b, dil):
    return F.conv2d(t, w_oihw, b, stride=1, padding=dil * (w_oihw.shape[2] - 1) // 2, dilation=dil)


def _params(method, weights, dtype, requires_grad):
    """{layer: (w OIHW tensor, b tensor)}"""
    out = {}
    for layer, (w, b) in layer_weights(method, weights).items():
        wt, bt = _t(w, dtype).permute(3, 2, 0, 1).contiguous(), _t(b, dtype)
        out[layer] = (wt.requires_grad_(requires_grad), bt.requires_grad_(requires_grad))
    return out


def _forward(method, P, t, tape=None):
    """the forward pass of deeplab_ref.forward on tensors; tape: a dict that receives every kept tensor (NCHW)"""
    def keep(name, v):
        if tape is not None:
            tape[name] = v
        return v

    keep("input", t)
    for name, kind, v in trunk_ops():
        if kind == "conv":
            t = F.relu(_conv(t, P[name][0], P[name][1], v))
        elif kind == "max":
            t = max_pool_same_t(t, v)
        else:
            t = avg_pool_same_t(t)
        keep(name, t)
    fc8 = None
    for sfx, rate in branches(method):
        u = keep("fc6" + sfx, F.relu(_conv(t, *P["fc6" + sfx], rate)))
        u = keep("fc7" + sfx, F.relu(_conv(u, *P["fc7" + sfx], 1)))
        y = _conv(u, *P["fc8" + sfx], 1)
        fc8 = y if fc8 is None else fc8 + y
    return fc8


def _hwio(w_oihw):
    return w_oihw.detach().permute(2, 3, 1, 0).contiguous().numpy()


def forward_tape(method, weights, x, dtype=torch.float64):
    """x (B, H, W, 3) -> ({tape name: NHWC array of `dtype`}, fc8 NHWC): the forward pass in `dtype`, everything kept"""
    tape = {}
    with torch.no_grad():
        fc8 = _forward(method, _params(method, weights, dtype, False), _nchw(x, dtype), tape)
    return {k: _nhwc(v) for k, v in tape.items()}, _nhwc(fc8)


def autograd_grads(method, weights, x, dfc8, dtype=torch.float64):
    """{layer: {'w': HWIO, 'b'}}: plain autograd of the whole forward pass in `dtype`, d loss / d fc8 = dfc8 (B, h, w, C)"""
    P = _params(method, weights, dtype, True)
    _forward(method, P, _nchw(x, dtype)).backward(_nchw(dfc8, dtype))
    return {layer: {"w": _hwio(w.grad), "b": b.grad.numpy().copy()} for layer, (w, b) in P.items()}


def _conv_back(x, w, b, dil, dz, want_dx):
    """the derivative of the (linear) convolution alone at input x: (dW OIHW, db, dx or None) for the gradient dz of its output"""
    x = x.detach().requires_grad_(want_dx)
    w, b = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
    _conv(x, w, b, dil).backward(dz)
    return w.grad, b.grad, x.grad if want_dx else None


def _pool_back(x, kind, stride, dy):
    x = x.detach().requires_grad_(True)
    (avg_pool_same_t(x) if kind == "avg" else max_pool_same_t(x, stride)).backward(dy)
    return x.grad


def chain_grads(method, weights, tape, dfc8, dtype=torch.float64):
    """The chain rule evaluated at `tape` ({name: NHWC array}, e.g. the device's own), in `dtype`: per layer, autograd of that one
    op on its kept input, the ReLU mask from its kept output.  -> {layer: {'w': HWIO, 'b'}} numpy arrays of `dtype`."""
    P = _params(method, weights, dtype, False)
    T = {k: _nchw(v, dtype) for k, v in tape.items()}
    g8 = _nchw(dfc8, dtype)
    out = {}

    def conv_layer(name, x_name, dil, g, relu=True, want_dx=True):
        dz = g * (T[name] > 0).to(dtype) if relu else g
        dw, db, dx = _conv_back(T[x_name], P[name][0], P[name][1], dil, dz, want_dx)
        out[name] = {"w": _hwio(dw), "b": db.numpy().copy()}
        return dx

    g = None
    for sfx, rate in branches(method):  # summed in the order _1 ... _4
        g7 = conv_layer("fc8" + sfx, "fc7" + sfx, 1, g8, relu=False)
        g6 = conv_layer("fc7" + sfx, "fc6" + sfx, 1, g7)
        g5 = conv_layer("fc6" + sfx, "pool5a", rate, g6)
        g = g5 if g is None else g + g5
    ops = trunk_ops()
    for i in range(len(ops) - 1, -1, -1):
        name, kind, v = ops[i]
        x_name = ops[i - 1][0] if i > 0 else "input"
        g = conv_layer(name, x_name, v, g, want_dx=i > 0) if kind == "conv" else _pool_back(T[x_name], kind, v, g)
    return out


def layer_ratio(got, ref):
    """{layer: (max|dw| / max|ref w|, max|db| / max|ref b|)} of two gradient dicts"""
    out = {}
    for layer in ref:
        r = []
        for which in ("w", "b"):
            a, b = np.asarray(got[layer][which], np.float64), np.asarray(ref[layer][which], np.float64)
            r.append(float(np.abs(a - b).max() / np.abs(b).max()))
        out[layer] = tuple(r)
    return out


# ---- float64 statements of the four per-layer entries on given float32 operands, each with the quantities its error bound needs --
def wgrad_ref(x, dz, k, dil):
    """x (N, H, W, Cin), dz (N, H, W, Cout) -> (dW HWIO, db, S = sum |x| |dz| per element of dW, n = in-image terms per tap (k, k),
    Sb = sum |dz| per channel), all float64"""
    f64 = torch.float64

    def dw_of(xa, dza):
        w = torch.zeros((dza.shape[3], xa.shape[3], k, k), dtype=f64, requires_grad=True)
        _conv(_nchw(xa, f64), w, None, dil).backward(_nchw(dza, f64))
        return _hwio(w.grad)

    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    n = dw_of(np.ones(x.shape[:3] + (1,)), np.ones(dz.shape[:3] + (1,)))[:, :, 0, 0]
    return dw_of(x, dz), dz.sum(axis=(0, 1, 2)), dw_of(np.abs(x), np.abs(dz)), np.rint(n), np.abs(dz).sum(axis=(0, 1, 2))


def dgrad_ref(dz, w, dil):
    """dz (N, H, W, Cout), w HWIO -> (dx (N, H, W, Cin), S = sum |dz| |w| per element), float64"""
    f64 = torch.float64
    k, cin = w.shape[0], w.shape[2]

    def dx_of(dza, wa):
        x = torch.zeros((dza.shape[0], cin) + dza.shape[1:3], dtype=f64, requires_grad=True)
        _conv(x, _t(wa, f64).permute(3, 2, 0, 1).contiguous(), None, dil).backward(_nchw(dza, f64))
        return _nhwc(x.grad)

    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    return dx_of(dz, w), dx_of(np.abs(dz), np.abs(w))


def pool_grad_ref(x, dy, avg, stride):
    """x (N, H, W, C), dy the pool's output size -> (dx, S = sum |terms| per element), float64; the tie rule is torch's: the first
    maximum in row-major window order"""
    f64 = torch.float64
    kind = "avg" if avg else "max"
    return (_nhwc(_pool_back(_nchw(x, f64), kind, stride, _nchw(dy, f64))),
            _nhwc(_pool_back(_nchw(x, f64), kind, stride, _nchw(np.abs(dy), f64))))


def pool_out_hw(H, W, stride):
    return -(-H // stride), -(-W // stride)
