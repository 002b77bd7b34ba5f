"""Non-finite inputs ("NaN and inf"): the poison values, where they are placed, the CONE of a placement and
the float64 reference semantics that tests/test_gpu_nonfinite.py holds the kernels to.  Plain numpy / torch.double: nothing here
touches the device.  tests/test_nonfinite_oracle.py pins what this file assumes of torch and of the suite's own oracles.

The cone of a poisoned element is the set of output cells that READ it: the cells whose reference value can change when the
element takes another value.  It is computed here from the operation's geometry alone, never from values.  A padded tap
counts as a read of the weight -- the reference's own GEMM multiplies the weight by the zero (0 * NaN = NaN in torch's conv2d
too: pinned in the oracle test) -- so the cone of a weight, a scale or a shift entry is its whole output channel.

Outside the cone the reference is the clean run's reference, exactly; inside it the tests assert finiteness and sign only."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import layer_ref as lr
from tests.helpers import bf16_round, f16_round
from wsscam import _lib

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
POISONS = {"nan": NAN, "pinf": PINF, "ninf": NINF}
CONTROL = 1e30  # finite: the IEEE-half modes report it as out of range, the modes with fp32's range compute with it
HALF_MODES = (_lib.PREC_F16, _lib.PREC_F16X3)
CARRY_MODES = (_lib.PREC_BF16, _lib.PREC_BF16X3, _lib.PREC_F32)  # bfloat16 and fp32 hold NaN / inf as they are

# the documented outcome per (entry point, precision): "L" loud, "P" propagate -- THE table of DESIGN.md section 5
def outcome(entry, prec, operand=None, cin=64):
    """operand / cin ("conv2d_nchw" only): the small-Cin forms (Cin <= 4) multiply a zero-weighted extra pixel per kernel row, so
    their INPUT is loud in bf16 / bf16x3 too (0 * NaN would leave the cone).
    entry: "conv2d_nchw", "pool" (the three forward pool entries), "gap_linear_sigmoid", "group_norm_nhwc" -> "L" / "P";
    the fp32-only entries ("cam_flip_add", "fc8_softmax", "pool_same_grad", "cls_loss", the gradient kernels, the SGD steps)
    are "P" whatever the precision; "net" (every whole-net forward), "net_create" and "load_params" are "L" in every precision."""
    if entry in ("net", "net_create", "load_params", "trainer_step"):
        return "L"
    if entry in ("cam_flip_add", "fc8_softmax", "pool_same_grad", "relu_bias_grad", "conv2d_wgrad", "conv2d_dgrad", "cls_loss", "seg_loss",
                 "irn_aff_loss", "seg_sgd", "irn_sgd"):
        return "P"
    if entry == "conv2d_nchw" and operand == "x" and cin <= 4 and prec != _lib.PREC_F32:
        return "L"
    if entry in ("conv2d_nchw", "pool", "gap_linear_sigmoid", "group_norm_nhwc"):
        return "L" if prec in HALF_MODES else "P"
    raise KeyError(entry)


def nonfinite(a):
    return ~np.isfinite(np.asarray(a))


def check_placement(cone, ref):
    """The two conditions every single-operation case meets (asserted by the callers on the CPU AND before a GPU case compares):
    at least half of the output lies outside the cone, and the reference has a non-finite cell -- all of them inside the cone."""
    cone = np.asarray(cone, dtype=bool)
    bad = nonfinite(ref)
    assert cone.shape == bad.shape, (cone.shape, bad.shape)
    assert 2 * int(cone.sum()) <= cone.size, "cone covers %d of %d cells" % (cone.sum(), cone.size)
    assert bad.any(), "vacuous case: the reference is finite everywhere"
    assert not (bad & ~cone).any(), "the reference is non-finite outside the cone at %s" % np.argwhere(bad & ~cone)[:4].tolist()


def assert_propagated(y, ref, cone, what=""):
    """Outcome P inside the cone: where the reference is NaN the device is NaN; where it is +-inf the device is NaN or the inf of
    that sign.  (A device NaN where the reference is finite -- relu(-inf) = 0, the split modes' inf - inf -- is allowed.)"""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rn = np.isnan(ref)
    miss = rn & ~np.isnan(y)
    assert not miss.any(), "%s: %d cells finite or inf where the reference is NaN, e.g. %s -> %r" % (
        what, miss.sum(), np.argwhere(miss)[:4].tolist(), y[miss][:4])
    ri = np.isinf(ref)
    ok = np.isnan(y) | (np.isinf(y) & (np.sign(y) == np.sign(ref)))
    miss = ri & ~ok
    assert not miss.any(), "%s: %d cells neither NaN nor the reference's inf, e.g. %s -> %r (reference %r)" % (
        what, miss.sum(), np.argwhere(miss)[:4].tolist(), y[miss][:4], ref[miss][:4])
    assert not (nonfinite(ref) & ~cone).any()


def assert_outside(y, ref, bound, cone, what=""):
    """Outside the cone: finite, and within the operation's bound of the reference."""
    out = ~np.asarray(cone, dtype=bool)
    y = np.asarray(y, dtype=np.float64)
    assert np.isfinite(y[out]).all(), "%s: non-finite outside the cone at %s" % (what, np.argwhere(out & nonfinite(y))[:4].tolist())
    with np.errstate(invalid="ignore"):  # (inf - inf inside the cone)
        err = np.abs(y - ref)
    bad = out & ~(err <= bound)
    assert not bad.any(), "%s: %d cells outside the cone beyond the bound, e.g. %s err %r bound %r" % (
        what, bad.sum(), np.argwhere(bad)[:4].tolist(), err[bad][:4], np.broadcast_to(bound, err.shape)[bad][:4])


# ---- conv layers (wsc_conv2d_nchw) ------------------------------------------------------------------------------------------
# (N, Cin, H, W, Cout, k, stride, pad): taken from tests/test_gpu_conv.py::SHAPES, where the kernel variant each selects is stated
CONV_SHAPES = [
    (2, 64, 9, 11, 72, 3, 1, 1),      # generic epilogue, partial column tile
    (2, 64, 19, 19, 64, 3, 1, 1),     # FAST epilogue and the LDS window
    (2, 64, 16, 16, 64, 1, 2, 0),     # one K-step, single buffer
    (3, 64, 21, 21, 64, 1, 1, 0),     # pointwise prologue
    (2, 3, 33, 37, 64, 3, 1, 1),      # small-Cin forms
    (2, 3, 65, 65, 64, 7, 2, 3),
]
CONV_BIG = (3, 512, 64, 64, 1024, 1, 1, 0)  # 256 x 256 tile, two 128-row groups (fp32 CPU oracle, as test_gpu_conv.py at this size)
CONV_PLACEMENTS = ("x_interior", "x_corner", "x_last", "weight", "scale", "shift", "residual")


def conv_out_hw(shape):
    N, Cin, H, W, Cout, k, stride, pad = shape
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_operands(shape):
    """x, w, scale, shift, residual as tests/test_gpu_conv.py::test_conv_layer draws them (a fixed seed per shape)"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    rng = np.random.default_rng(sum(int(v) * 31 ** i for i, v in enumerate(shape)) % (2 ** 31))
    x = rng.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k))).astype(np.float32)
    w *= (1.0 + 0.5 * np.arange(Cout, dtype=np.float32) / Cout)[:, None, None, None]
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    Ho, Wo = conv_out_hw(shape)
    res = rng.normal(0, 1, (N, Cout, Ho, Wo)).astype(np.float32)
    return {"x": x, "w": w, "scale": scale, "shift": shift, "residual": res}


def conv_place(shape, placement):
    """-> (operand name, index tuple) of the poisoned element"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    Ho, Wo = conv_out_hw(shape)
    # an interior pixel that some window reads (a strided 1 x 1 layer reads the even pixels only)
    hi, wi = (H // 2) // stride * stride, (W // 2) // stride * stride
    return {
        "x_interior": ("x", (0, Cin // 2, hi, wi)),
        "x_corner": ("x", (0, 0, 0, 0)),  # (padding taps in its windows)
        "x_last": ("x", (N - 1, Cin - 1, (H - 1) // stride * stride if k == 1 else H - 1, (W - 1) // stride * stride if k == 1 else W - 1)),
        "weight": ("w", (Cout // 3, Cin // 2, k // 2, k - 1)),
        "scale": ("scale", (5,)),
        "shift": ("shift", (Cout - 1,)),
        "residual": ("residual", (N - 1, Cout - 1, Ho - 1, Wo - 1)),
    }[placement]


def conv_cone(shape, placement):
    """bool (N, Cout, Ho, Wo): the cells that read the poisoned element"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    Ho, Wo = conv_out_hw(shape)
    name, idx = conv_place(shape, placement)
    cone = np.zeros((N, Cout, Ho, Wo), dtype=bool)
    if name == "x":
        n, _, h, w = idx
        for ho in range(Ho):
            if not 0 <= h - (ho * stride - pad) < k:
                continue
            for wo in range(Wo):
                if 0 <= w - (wo * stride - pad) < k:
                    cone[n, :, ho, wo] = True
    elif name == "residual":
        cone[idx] = True
    else:  # a weight, a scale or a shift entry: its output channel
        cone[:, idx[0]] = True
    return cone


def conv_poisoned(ops, shape, placement, value):
    name, idx = conv_place(shape, placement)
    out = dict(ops)
    out[name] = ops[name].copy()
    out[name][idx] = value
    return out


def conv_ref(ops, shape, use_res, relu, prec=None, dtype=torch.float64):
    """relu(conv(x, w) scale + shift + residual) in `dtype`.  prec bf16 / f16: the operands the one-plane modes hold (rounded
    like test_conv_layer rounds them; a non-finite value is kept as it is -- the rounding helpers are for numbers)."""
    N, Cin, H, W, Cout, k, stride, pad = shape

    def rnd(a):
        if prec not in (_lib.PREC_BF16, _lib.PREC_F16):
            return a
        fin = np.isfinite(a)
        r = (bf16_round if prec == _lib.PREC_BF16 else f16_round)(np.where(fin, a, 0).astype(np.float32))
        return np.where(fin, r, a).astype(np.float32)

    x, w, res = rnd(ops["x"]), rnd(ops["w"]), rnd(ops["residual"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    with torch.no_grad():
        y = F.conv2d(t(x), t(w), stride=stride, padding=pad)
        y = y * t(ops["scale"])[None, :, None, None] + t(ops["shift"])[None, :, None, None]
        if use_res:
            y = y + t(res)
        if relu:
            y = torch.relu(y)
    return y.numpy().astype(np.float64)


def conv_bound(prec, ref, ops, shape, use_res, cone=None, mx_clean=None):
    """The bound of tests/test_gpu_conv.py::test_conv_layer (16-bit modes) / tests/test_gpu_f32.py (PREC_F32) for a reference
    `ref`.  max|ref|: outside `cone` the CLEAN reference's maximum `mx_clean` -- those cells are the clean run's, and a 1e30 in
    the cone must not widen their bound; inside the cone (the finite control) the maximum over the finite cells of `ref`."""
    fin = np.isfinite(ref)
    mx = np.abs(ref[fin]).max()
    if cone is not None:
        mx = np.where(cone, mx, mx_clean)
    a = np.where(fin, np.abs(ref), 0.0)
    if prec == _lib.PREC_BF16:
        return 2.0 ** -8 * a + 2e-3 * mx
    if prec == _lib.PREC_F16:
        return 2.0 ** -11 * a + 3e-4 * mx
    if prec == _lib.PREC_BF16X3:
        return np.zeros_like(ref) + 1e-4 * mx
    if prec == _lib.PREC_F16X3:
        return np.zeros_like(ref) + 4e-6 * mx
    # PREC_F32: (K + 8) 2^-24 A, A = conv(|x|, |w|) |scale| + |shift| + |residual|
    N, Cin, H, W, Cout, k, stride, pad = shape
    fz = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0).astype(np.float64)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    with torch.no_grad():
        A = F.conv2d(t(fz(ops["x"])), t(fz(ops["w"])), stride=stride, padding=pad).numpy()
    A = A * fz(ops["scale"])[None, :, None, None] + fz(ops["shift"])[None, :, None, None]
    if use_res:
        A = A + fz(ops["residual"])
    return (Cin * k * k + 8) * 2.0 ** -24 * A


def conv_shifted_ref(ops0, raw, shape, placement, value, prec, dtype=np.float64, pre=None):
    """The reference of a 1 x 1 / stride 1 / pad 0 layer (residual, ReLU) whose element `placement` holds `value`, from the clean
    layer's accumulator raw = conv(x, w) and clean operands ops0 (already what the precision holds): outside the cone the clean
    value; in the cone the clean pre-activation plus the one changed term -- (value - old) times what multiplies it -- so an inf
    takes the sign of its product and a NaN stays a NaN.  Computed, not painted.  pre: the clean pre-activation where the caller
    keeps it (it is copied)."""
    N, Cin, H, W, Cout, k, stride, pad = shape
    assert (k, stride, pad) == (1, 1, 0)
    name, idx = conv_place(shape, placement)
    v = np.float32(value)
    if prec == _lib.PREC_BF16 and name in ("x", "w", "residual") and np.isfinite(v):
        v = bf16_round(np.array([v], np.float32))[0]
    v = dtype(v)
    x, w, scale, shift, res = (np.asarray(ops0[n], dtype) for n in ("x", "w", "scale", "shift", "residual"))
    s4, b4 = scale[None, :, None, None], shift[None, :, None, None]
    pre = np.asarray(raw, dtype) * s4 + b4 + res if pre is None else pre.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if name == "x":
            n, ci, h, ww = idx
            pre[n, :, h, ww] += (v - x[n, ci, h, ww]) * w[:, ci, 0, 0] * scale
        elif name == "w":
            co, ci = idx[0], idx[1]
            pre[:, co] += (v - w[co, ci, 0, 0]) * x[:, ci] * scale[co]
        elif name == "scale":
            pre[:, idx[0]] += (v - scale[idx[0]]) * np.asarray(raw, dtype)[:, idx[0]]
        elif name == "shift":
            pre[:, idx[0]] += v - shift[idx[0]]
        else:
            pre[idx] += v - res[idx]
    return np.where(np.isnan(pre), pre, np.maximum(pre, 0)).astype(np.float64)


# ---- pools ------------------------------------------------------------------------------------------------------------------
# (H, W, stride): N = 1, C = 64, k = 3
POOL_GEOMS = [(9, 11, 2), (13, 13, 2), (9, 11, 1), (13, 13, 1)]
POOL_PLACEMENTS = ("shared", "border")


def pool_place(H, W, stride, placement):
    """(h, w, c) of the poisoned cell: one that two windows share, or a border cell"""
    return (H // 2 - (H // 2) % 2 + 1, W // 2 - (W // 2) % 2 + 1, 7) if placement == "shared" else (0, W - 1, 63)


def pool_windows(H, k, stride, rule, pad=1):
    """[(first, last + 1)] in-image rows of every window of an axis; rule "torch" (pad before = pad) or "same" (TF SAME)"""
    if rule == "torch":
        out, before = (H + 2 * pad - k) // stride + 1, pad
    else:
        out = -(-H // stride)
        before = max((out - 1) * stride + k - H, 0) // 2
    return [(max(o * stride - before, 0), min(o * stride - before + k, H)) for o in range(out)]


def pool_cone(H, W, C, k, stride, rule, cell):
    h, w, c = cell
    rows, cols = pool_windows(H, k, stride, rule), pool_windows(W, k, stride, rule)
    cone = np.zeros((1, len(rows), len(cols), C), dtype=bool)
    for i, (a, b) in enumerate(rows):
        for j, (p, q) in enumerate(cols):
            if a <= h < b and p <= w < q:
                cone[0, i, j, c] = True
    return cone


def pool_ref(x, k, stride, rule, avg):
    """NHWC float64 pool over the in-image taps: their maximum (NaN carried: np.max), or their average"""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, C = x.shape
    rows, cols = pool_windows(H, k, stride, rule), pool_windows(W, k, stride, rule)
    y = np.empty((N, len(rows), len(cols), C))
    for i, (a, b) in enumerate(rows):
        for j, (p, q) in enumerate(cols):
            win = x[:, a:b, p:q, :].reshape(N, -1, C)
            y[:, i, j, :] = win.mean(axis=1) if avg else win.max(axis=1)
    return y


def pool_grad_ref(x, dy, k, stride, avg):
    """The gradient of the TF-SAME pool with respect to x (float64): dy to the first maximum of every window in row-major
    window order, or dy / (in-image taps) to every tap"""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    N, H, W, C = x.shape
    rows, cols = pool_windows(H, k, stride, "same"), pool_windows(W, k, stride, "same")
    dx = np.zeros_like(x)
    for i, (a, b) in enumerate(rows):
        for j, (p, q) in enumerate(cols):
            if avg:
                dx[:, a:b, p:q, :] += dy[:, i:i + 1, j:j + 1, :] / ((b - a) * (q - p))
                continue
            win = x[:, a:b, p:q, :].reshape(N, -1, C)
            arg = win.argmax(axis=1)  # (the first maximum)
            for n in range(N):
                for c in range(C):
                    r, s = divmod(int(arg[n, c]), q - p)
                    dx[n, a + r, p + s, c] += dy[n, i, j, c]
    return dx


def pool_grad_cone(x, k, stride, avg, cell):
    """the input cells that receive dy[0, i, j, c] (cell = (i, j, c))"""
    i, j, c = cell
    N, H, W, C = x.shape
    rows, cols = pool_windows(H, k, stride, "same"), pool_windows(W, k, stride, "same")
    (a, b), (p, q) = rows[i], cols[j]
    cone = np.zeros(x.shape, dtype=bool)
    if avg:
        cone[0, a:b, p:q, c] = True
    else:
        r, s = divmod(int(np.asarray(x, dtype=np.float64)[0, a:b, p:q, c].reshape(-1).argmax()), q - p)
        cone[0, a + r, p + s, c] = True
    return cone


# ---- relu-like references of the heads -------------------------------------------------------------------------------------
def fc8_softmax_ref(logits, min_prob):
    """softmax over the last axis + min_prob, renormalised, float64 (build_sp_softmax)"""
    z = torch.from_numpy(np.asarray(logits, dtype=np.float64))
    p = torch.softmax(z, dim=-1) + min_prob
    return (p / p.sum(dim=-1, keepdim=True)).numpy()


def relu_bias_grad_ref(y, dy, scale=1.0):
    """dz = dy scale [y > 0], db = column sums of dz (float64)"""
    dz = np.where(np.asarray(y) > 0, np.asarray(dy, dtype=np.float64) * np.float64(np.float32(scale)), 0.0)
    return dz, dz.sum(axis=0)


def precision_values(x, prec):
    """layer_ref.as_precision on the finite values; a non-finite value stays what it is"""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    return np.where(fin, lr.as_precision(np.where(fin, x, 0).astype(np.float32), prec), x).astype(np.float32)
