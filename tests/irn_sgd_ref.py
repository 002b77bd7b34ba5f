"""TEST INFRASTRUCTURE ONLY (oracle) -- the update half of an IRNet training step (step/train_irn.py:86-90, 127-129) and the
closing dp_mean pass (148-164), restated on the host.

    poly_lrs(lr, max_step, power, global_step)   the two rates PolyOptimizer sets before step `global_step`, Python doubles
    sgd_step32(p, g, m, boundary, lr_edge, lr_dp, wd, mo)   THE DEFINITION the device is held to bit for bit: torch.optim.SGD
                       (dampening 0, no Nesterov) with every product and sum rounded to float32 on its own, no fused multiply-add;
                       the scalars are cast to float32 first, the cast torch applies for fp32 tensors.  m starts at +0.0.
    sgd_step64         the same expressions in float64 (against torch.double)
    layout(sd, arch) / flat_params(sd, arch) / unflatten(flat, sd, arch)   the flat layout of wsc_irn_grad_layout from
                       irn_grad_ref.param_names: conv weights as [Cin][Cout], no gaps; boundary(sd, arch) = the first dp float
    channel_mean64(x)  torch.mean(x, dim=(0, 2, 3)) in float64;  dp_mean64(batches, shift) the closing pass

tests/test_irn_sgd_oracle.py measures the two constants below against torch on the CPU.

R32_SGD   max |p_restated - p_torch| / max(1, max|p|) over the ResNet50 head layout after 6 and after 9 steps at max_step = 7,
          random N(0, 1) gradients: torch's vector body fuses a + alpha b where the restatement rounds twice.
R32_MEAN  the same ratio for float32 torch.mean(dp, (0, 2, 3)) + stack-mean against the float64 oracle."""
import numpy as np

from tests import irn_grad_ref

R32_SGD = 1.66e-7  # after 6 steps (1.56e-7 after 9); 47 - 50 % of the elements differ from torch in some bit
R32_MEAN = 3.17e-8  # three batches of (3, 2, 17, 17)

F = np.float32


def poly_lrs(lr, max_step, power, global_step):
    """(lr_edge, lr_dp) of the step taken at `global_step`: lr0 (1 - t / max_step) ** power with t = global_step while it is below
    max_step; from max_step on the groups keep the last value that was set (t = max_step - 1)."""
    t = min(int(global_step), int(max_step) - 1)
    mult = (1 - t / max_step) ** power
    return float(lr) * mult, (10 * float(lr)) * mult


def _lr_vector(n, boundary, lr_edge, lr_dp, dtype):
    lr = np.full((n,), dtype(lr_dp), dtype)
    lr[:boundary] = dtype(lr_edge)
    return lr


def sgd_step32(p, g, m, boundary, lr_edge, lr_dp, wd, mo):
    """-> (p, m) after one step; float32 arrays in, every operation one float32 rounding (numpy does not fuse)"""
    p, g, m = np.asarray(p, F), np.asarray(g, F), np.asarray(m, F)
    with np.errstate(under="ignore"):
        t = g + F(wd) * p
        m2 = F(mo) * m + t
        p2 = p - _lr_vector(p.size, boundary, F(lr_edge), F(lr_dp), F) * m2
    assert t.dtype == F and m2.dtype == F and p2.dtype == F
    return p2, m2


def sgd_step64(p, g, m, boundary, lr_edge, lr_dp, wd, mo):
    p, g, m = np.asarray(p, np.float64), np.asarray(g, np.float64), np.asarray(m, np.float64)
    m2 = mo * m + (g + wd * p)
    return p - _lr_vector(p.size, boundary, lr_edge, lr_dp, np.float64) * m2, m2


def _np(v):
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)


def layout(sd, arch):
    """[(name, offset, torch shape, is conv weight)] and the number of floats"""
    edge, dp = irn_grad_ref.param_names(arch)
    out, at = [], 0
    for name in edge + dp:
        shape = tuple(_np(sd[name]).shape)
        out.append((name, at, shape, len(shape) == 4))
        at += int(np.prod(shape))
    return out, at


def boundary(sd, arch):
    edge, _ = irn_grad_ref.param_names(arch)
    return sum(int(np.prod(_np(sd[n]).shape)) for n in edge)


def flat_params(sd, arch, dtype=np.float32):
    lay, n = layout(sd, arch)
    flat = np.empty((n,), dtype)
    for name, at, shape, conv in lay:
        v = _np(sd[name]).astype(dtype)
        if conv:
            v = v.reshape(shape[0], shape[1]).T
        flat[at:at + v.size] = v.reshape(-1)
    return flat


def unflatten(flat, sd, arch):
    out = {}
    for name, at, shape, conv in layout(sd, arch)[0]:
        v = np.asarray(flat)[at:at + int(np.prod(shape))]
        if conv:
            v = v.reshape(shape[1], shape[0]).T
        out[name] = np.ascontiguousarray(v.reshape(shape)).copy()
    return out


def channel_mean64(x):
    return np.asarray(x, np.float64).mean(axis=(0, 2, 3))


def dp_mean64(batches, shift=None):
    """the closing loop on raw dp_out batches [N][2][H][W]: per batch the channel mean minus the current mean shift, then the
    mean of the stacked batch means, float64"""
    s = np.zeros(2, np.float64) if shift is None else np.asarray(shift, np.float32).astype(np.float64)
    means = np.stack([channel_mean64(b) - s for b in batches])
    return means.sum(axis=0) / len(batches)
