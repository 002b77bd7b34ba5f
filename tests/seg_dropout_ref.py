"""Oracle of the dropout sites of the SEC / DSRG training graph (drop6 / drop7 behind fc6 / fc7) under the project's own
counter-based contract (include/wsscam.h): a numpy Philox4x32-10, the keep-masks, the fp32 statement of the
kernel, and the torch forward / backward passes of tests/deeplab_grad_ref.py with explicit mask multiplication.

The contract: element i (the linear NHWC index of the [B][h][w][Cout] tensor) draws from counter (low(i >> 2), high(i >> 2), step,
site) under key (seed low, seed high) and takes output word i & 3; u = float32(word >> 8) 2^-24; keep iff u >= drop_prob (both
float32); d = float32(y * scale) where kept, +0.0 where dropped, scale = float32(1) / (float32(1) - float32(drop_prob)).  Branch k
(0-based) uses site 2 k behind fc6 and 2 k + 1 behind fc7."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.deeplab_grad_ref import _conv, _conv_back, _hwio, _nchw, _nhwc, _params, _pool_back, branches, trunk_ops
from tests.deeplab_ref import avg_pool_same_t, max_pool_same_t

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two ints -> four uint32 arrays, Random123's philox4x32 with 10 rounds"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # (< 2^64: exact in uint64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def site_of(branch, layer):
    """branch k (0-based), layer 6 or 7 -> the site of drop6_k / drop7_k"""
    return 2 * branch + (layer - 6)


def uniform(n, seed, step, site, first=0):
    """float32 (n,): u of the elements first ... first + n - 1"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(first)
    blk = i >> np.uint64(2)
    lo, idx = np.unique(blk, return_inverse=True)
    words = philox4x32_10((lo & MASK32, lo >> np.uint64(32), int(step), int(site)), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    word = np.stack(words, axis=1)[idx, (i & np.uint64(3)).astype(np.int64)]
    return (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(shape, drop_prob, seed, step, site, first=0):
    """bool array of `shape` (C order = the linear NHWC index): True where the element is kept"""
    n = int(np.prod(shape))
    return (uniform(n, seed, step, site, first) >= np.float32(drop_prob)).reshape(shape)


def scale_of(drop_prob):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(drop_prob))


def dropout_f32(x, drop_prob, seed, step, site, first=0):
    """float32 x (any shape, C order) -> (d, keep): the kernel's statement on plain float32"""
    x = np.asarray(x, dtype=np.float32)
    keep = keep_mask(x.shape, drop_prob, seed, step, site, first)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.where(keep, x * scale_of(drop_prob), np.float32(0.0)).astype(np.float32)
    return d, keep


def _masks(method, shapes, drop_prob, seed, step, dtype):
    """{tape name: NCHW tensor of mask * scale} for every fc6* / fc7*; shapes: {tape name: NHWC shape}"""
    out = {}
    s = float(scale_of(drop_prob))
    for k, (sfx, _) in enumerate(branches(method)):
        for layer in (6, 7):
            name = "fc%d%s" % (layer, sfx)
            m = keep_mask(shapes[name], drop_prob, seed, step, site_of(k, layer))
            out[name] = _nchw(m.astype(np.float64) * s, dtype)
    return out


def _forward_drop(method, P, t, drop, tape=None):
    """deeplab_grad_ref._forward with the dropout sites: drop = (drop_prob, seed, step)"""
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
    B, _, h, w = t.shape
    shapes = {}
    for sfx, _ in branches(method):
        for layer in ("fc6", "fc7"):
            shapes[layer + sfx] = (B, h, w, P[layer + sfx][0].shape[0])
    masks = _masks(method, shapes, drop[0], drop[1], drop[2], t.dtype)
    fc8 = None
    for sfx, rate in branches(method):
        u = keep("fc6" + sfx, F.relu(_conv(t, *P["fc6" + sfx], rate)) * masks["fc6" + sfx])
        u = keep("fc7" + sfx, F.relu(_conv(u, *P["fc7" + sfx], 1)) * masks["fc7" + sfx])
        y = _conv(u, *P["fc8" + sfx], 1)
        fc8 = y if fc8 is None else fc8 + y
    return fc8


def forward_tape_drop(method, weights, x, drop, dtype=torch.float64):
    """deeplab_grad_ref.forward_tape with dropout: the fc6* / fc7* entries are the dropped, scaled activations"""
    tape = {}
    with torch.no_grad():
        fc8 = _forward_drop(method, _params(method, weights, dtype, False), _nchw(x, dtype), drop, tape)
    return {k: _nhwc(v) for k, v in tape.items()}, _nhwc(fc8)


def autograd_grads_drop(method, weights, x, dfc8, drop, dtype=torch.float64):
    """deeplab_grad_ref.autograd_grads of the forward pass with explicit mask multiplication"""
    P = _params(method, weights, dtype, True)
    _forward_drop(method, P, _nchw(x, dtype), drop).backward(_nchw(dfc8, dtype))
    return {layer: {"w": _hwio(w.grad), "b": b.grad.numpy().copy()} for layer, (w, b) in P.items()}


def chain_grads_drop(method, weights, tape, dfc8, drop_prob, dtype=torch.float64):
    """deeplab_grad_ref.chain_grads on a tape of a dropout forward pass: dz = g * scale * (T > 0) at fc6 / fc7 (the tape entry is
    > 0 exactly where the unit was kept and its ReLU output positive), everything else unchanged.  No mask is read."""
    P = _params(method, weights, dtype, False)
    T = {k: _nchw(v, dtype) for k, v in tape.items()}
    g8 = _nchw(dfc8, dtype)
    s = float(scale_of(drop_prob))
    out = {}

    def conv_layer(name, x_name, dil, g, relu=True, want_dx=True, scale=1.0):
        dz = g * scale * (T[name] > 0).to(dtype) if relu else g
        dw, db, dx = _conv_back(T[x_name], P[name][0], P[name][1], dil, dz, want_dx)
        out[name] = {"w": _hwio(dw), "b": db.numpy().copy()}
        return dx

    g = None
    for sfx, rate in branches(method):
        g7 = conv_layer("fc8" + sfx, "fc7" + sfx, 1, g8, relu=False)
        g6 = conv_layer("fc7" + sfx, "fc6" + sfx, 1, g7, scale=s)
        g5 = conv_layer("fc6" + sfx, "pool5a", rate, g6, scale=s)
        g = g5 if g is None else g + g5
    ops = trunk_ops()
    for i in range(len(ops) - 1, -1, -1):
        name, kind, v = ops[i]
        x_name = ops[i - 1][0] if i > 0 else "input"
        g = conv_layer(name, x_name, v, g, want_dx=i > 0) if kind == "conv" else _pool_back(T[x_name], kind, v, g)
    return out
