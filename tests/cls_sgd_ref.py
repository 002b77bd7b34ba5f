"""Reference of the update half of a 01_train step (csrc/sgd.hip, csrc/repack.hip; wsc_cls_param_layout, wsc_cls_sgd_step, wsc_net_cls_load_params;
cls_train.ClsTrainer, step_lr, cyclic_lr), in numpy.

  sgd_step32     Keras 2.2 optimizers.SGD(lr, momentum, decay=0.0, nesterov).get_updates restated with ONE np.float32 operation per
                 rounding: v = momentum m - lr g; m = v; p = (p + momentum v) - lr g (nesterov) / p + v; lr g formed once.  This is
                 the definition the device is held to bit for bit.
  sgd_step64     the same expressions in float64 (what the float32 restatement is an approximation of)
  layout         the training layout from the state dict alone: per conv `.weight` ([3][3][Cin][Cout]) and `.bias`, then its
                 BatchNorm's `.weight` / `.bias`; then the classifier's Linear, the first C rows as they lie, and its bias if any
  flat_params    a state dict in that layout
  fold           BatchNorm's inference scale / shift as net.hip's fold_bn forms them: double, each rounded to float once"""
import numpy as np

from tests import cls_grad_ref as gref

f32 = np.float32


def sgd_step32(p, g, m, lr, momentum, nesterov=True):
    """-> (p, m) float32 arrays"""
    p, g, m = np.asarray(p, f32), np.asarray(g, f32), np.asarray(m, f32)
    lr, mo = f32(lr), f32(momentum)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        lg = (lr * g).astype(f32)
        v = ((mo * m).astype(f32) - lg).astype(f32)
        if nesterov:
            p = ((p + (mo * v).astype(f32)).astype(f32) - lg).astype(f32)
        else:
            p = (p + v).astype(f32)
    return p, v


def sgd_step64(p, g, m, lr, momentum, nesterov=True):
    p, g, m = np.asarray(p, np.float64), np.asarray(g, np.float64), np.asarray(m, np.float64)
    v = momentum * m - lr * g
    return (p + momentum * v - lr * g) if nesterov else (p + v), v


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def layout(sd, root, C):
    """-> ([(name, offset, shape as it lies)], param_elems, grad_elems)"""
    out, at = [], 0
    for name in gref.param_names(root, sd):
        shape = tuple(_np(sd[name]).shape)
        lies = (3, 3, shape[1], shape[0]) if len(shape) == 4 else shape
        out.append((name, at, lies))
        at += int(np.prod(lies))
    grad_elems = at
    F = _np(sd[root + ".classifier.0.weight"]).shape[1]
    out.append((root + ".classifier.0.weight", at, (C, F)))
    at += C * F
    if root + ".classifier.0.bias" in sd:
        out.append((root + ".classifier.0.bias", at, (C,)))
        at += C
    return out, at, grad_elems


def flat_params(sd, root, C):
    ent, n, _ = layout(sd, root, C)
    flat = np.empty(n, f32)
    for name, at, lies in ent:
        v = _np(sd[name]).astype(f32)
        v = v.transpose(2, 3, 1, 0) if v.ndim == 4 else (v[:C] if ".classifier." in name else v)
        assert v.shape == lies, (name, v.shape, lies)
        flat[at:at + v.size] = v.reshape(-1)
    return flat


def unflatten(flat, sd, root, C):
    """the inverse: {name: array in torch's shape}"""
    out = {}
    for name, at, lies in layout(sd, root, C)[0]:
        v = np.asarray(flat[at:at + int(np.prod(lies))], f32).reshape(lies)
        out[name] = np.ascontiguousarray(v.transpose(3, 2, 0, 1) if len(lies) == 4 else v)
    return out


def fold(gamma, beta, mean, var, eps=1e-3):
    """(s2, b2) float32: sc = gamma / sqrt(var + eps), b = beta - mean sc in double, each rounded once (numpy's float64 division
    and square root are IEEE's correctly rounded ones, as the C library's)"""
    g, b, mu, v = (np.asarray(a, f32).astype(np.float64) for a in (gamma, beta, mean, var))
    sc = g / np.sqrt(v + np.float64(eps))
    return sc.astype(f32), (b - mu * sc).astype(f32)
