"""numpy restatement of the update half of a SEC / DSRG training step (03a_sec-dsrg/model.py:379-404, 491-504; csrc/sgd.hip, csrc/repack.hip):

    accumulate   t = grad + weight_decay * param on weights (every layer, fc8 included), t = grad on biases;
                 t = mult * t with mult 1 (weights), 2 (biases), 10 (fc8 weights), 20 (fc8 biases);  accum += t / accum_num
    apply        mom = mom * momentum + accum;  param = param - lr * mom;  accum = +0.0 (clear)      [ApplyMomentum, no Nesterov]
    l2           sum over the layers of sum(w^2) / 2

in float32 with ONE np.float32 operation per rounding (the device's bits), and a float64 twin.  Everything works on the flat layout
of wsc_seg_grad_layout: per layer w in HWIO, then b, no gaps, the layers in execution order."""
import numpy as np

from tests import deeplab_ref


def layout_of(method, weights):
    """{layer: {'k', 'Cin', 'Cout', 'w_off', 'b_off'}}, the float count: what wsc_seg_grad_layout reports for these weights"""
    out, n = {}, 0
    for layer in deeplab_ref.layer_names(method):
        k, _, cin, cout = np.shape(weights[layer]["w"])
        out[layer] = {"k": k, "Cin": cin, "Cout": cout, "w_off": n, "b_off": n + k * k * cin * cout}
        n += k * k * cin * cout + cout
    return out, n


def segments(layout):
    """[(name, start, stop, mult, decay)] in offset order: one segment per w and per b"""
    segs = []
    for layer, e in layout.items():
        fc8 = layer.startswith("fc8")
        nw = e["k"] * e["k"] * e["Cin"] * e["Cout"]
        segs.append((layer + ".w", e["w_off"], e["w_off"] + nw, 10.0 if fc8 else 1.0, True))
        segs.append((layer + ".b", e["b_off"], e["b_off"] + e["Cout"], 20.0 if fc8 else 2.0, False))
    return segs


def flatten(layout, n, weights):
    flat = np.empty((n,), np.float32)
    for layer, e in layout.items():
        w = np.asarray(weights[layer]["w"], np.float32).reshape(-1)
        flat[e["w_off"]:e["w_off"] + w.size] = w
        flat[e["b_off"]:e["b_off"] + e["Cout"]] = np.asarray(weights[layer]["b"], np.float32).reshape(-1)
    return flat


def unflatten(layout, flat):
    out = {}
    for layer, e in layout.items():
        shape = (e["k"], e["k"], e["Cin"], e["Cout"])
        out[layer] = {"w": flat[e["w_off"]:e["w_off"] + int(np.prod(shape))].reshape(shape).copy(),
                      "b": flat[e["b_off"]:e["b_off"] + e["Cout"]].copy()}
    return out


def accumulate(segs, param, grad, accum, weight_decay, accum_num, dtype=np.float32):
    """-> the new accumulator (a new array); every operation one rounding of `dtype`"""
    f = dtype
    param, grad = np.asarray(param, f), np.asarray(grad, f)
    out = np.array(accum, f)
    for _, a, b, mult, decay in segs:
        t = grad[a:b]
        if decay:
            t = t + f(weight_decay) * param[a:b]
        t = f(mult) * t
        out[a:b] = out[a:b] + t / f(accum_num)
    return out


def apply(param, accum, mom, lr, momentum, clear_accum=True, dtype=np.float32):
    """-> (param, accum, mom), new arrays"""
    f = dtype
    mom = np.asarray(mom, f) * f(momentum) + np.asarray(accum, f)
    param = np.asarray(param, f) - f(lr) * mom
    accum = np.zeros_like(mom) if clear_accum else np.array(accum, f)
    return param, accum, mom


def l2(segs, param):
    """loss['l2'] in float64"""
    return sum(0.5 * float(np.sum(np.asarray(param[a:b], np.float64) ** 2)) for _, a, b, _, decay in segs if decay)


def lr_at(epoch, base_lr=1e-4, lr_decay=0.5, lr_step=4):
    """model.py:493, stored in a float32 variable"""
    return np.float32(base_lr * lr_decay ** (epoch // lr_step))
