"""float64 oracle of the SEC / DSRG loss head (03a_sec-dsrg/SEC.py:363-465, DSRG.py:459-518) and of its gradient.

A torch restatement of the formulas of include/wsscam.h (wsc_seg_loss): torch.sort for the rank pooling, torch.amax for the
maximum (its gradient is split equally among tied maxima, TensorFlow's reduce_max rule).  float32 inputs are promoted to float64;
min_prob is the float32 the C ABI receives, promoted.

The gradient oracle is autograd with p = fc8-softmax as the leaf, EXCEPT for the rank-pooling terms loss_1 and loss_3: autograd's
choice of who gets which weight inside a group of equal values is unspecified, so those weights are placed by
np.argsort(kind='stable') -- among equal values the lower pixel index gets the lower rank.  On maps without ties the two agree
(tests/test_seg_loss_oracle.py holds them to each other).  g_z = dL/dfc8 comes from g_p by the chain rule through
build_sp_softmax, grad_fc8(); the same test holds that formula to autograd from the logits."""
import numpy as np
import torch

Q_FG, Q_BG = 0.996, 0.999
KEYS = ("seed", "constrain", "expand", "loss_1", "loss_2", "loss_3", "norm", "seed_bg", "seed_fg")


def rank_weights(n, q):
    """The reference's expression (SEC.py:415-418), cast as TensorFlow casts a numpy constant in float32 arithmetic."""
    w64 = np.array([q ** i for i in range(n - 1, -1, -1)])
    return w64.astype(np.float32), np.float32(np.sum(w64))


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.float64)


def sp_softmax(z, m):
    """build_sp_softmax (SEC.py:246-249) on a torch tensor"""
    e = torch.exp(z - z.amax(dim=3, keepdim=True))
    p = e / e.sum(dim=3, keepdim=True) + m
    return p / p.sum(dim=3, keepdim=True)


def grad_fc8(p, g_p, m):
    """s = p (1 + C m) - m;  g_z = s (g_p - sum_j g_p,j s_j) / (1 + C m)"""
    C = p.shape[3]
    s = p * (1 + C * m) - m
    return s * (g_p - (g_p * s).sum(3, keepdims=True)) / (1 + C * m)


def _tables(n):
    w_fg, z_fg = rank_weights(n, Q_FG)
    w_bg, z_bg = rank_weights(n, Q_BG)
    return t64(w_fg), float(z_fg), t64(w_bg), float(z_bg)


def terms(method, p, crf, cues, labels=None):
    """p (B, h, w, C) float64 torch tensor (may require grad); crf, cues, labels float64 tensors
    -> ({name: scalar tensor}, {name: sum of the magnitudes of the terms the value is the sum of})"""
    B, h, w, C = p.shape
    n = h * w
    q = torch.exp(crf)
    out, mag = {}, {}
    if method == "SEC":
        count = torch.clamp(cues.sum(dim=(1, 2, 3)), min=1e-5)
        t = cues * torch.log(p)
        out["seed"] = -(t.sum(dim=(1, 2, 3)) / count).mean()
        mag["seed"] = float((t.detach().abs().sum(dim=(1, 2, 3)) / count).mean())
        t = q * torch.log(q / p)
        out["constrain"] = t.sum() / (B * n)
        mag["constrain"] = float(t.detach().abs().sum() / (B * n))
        w_fg, z_fg, w_bg, z_bg = _tables(n)
        maps = p.reshape(B, n, C)
        stat = (labels.reshape(B, C)[:, 1:] > 0).to(torch.float64)
        mean = (torch.sort(maps[:, :, 1:], dim=1)[0] * w_fg.reshape(1, n, 1)).sum(1) / z_fg
        bgmean = (torch.sort(maps[:, :, 0], dim=1)[0] * w_bg.reshape(1, n)).sum(1) / z_bg
        vmax = torch.amax(maps[:, :, 1:], dim=1)
        t = stat * torch.log(mean) / torch.clamp(stat.sum(1, keepdim=True), min=1e-5)
        out["loss_1"], mag["loss_1"] = -t.sum(1).mean(), float(t.detach().abs().sum(1).mean())
        t = (1 - stat) * torch.log(1 - vmax) / torch.clamp((1 - stat).sum(1, keepdim=True), min=1e-5)
        out["loss_2"], mag["loss_2"] = -t.sum(1).mean(), float(t.detach().abs().sum(1).mean())
        t = torch.log(bgmean)
        out["loss_3"], mag["loss_3"] = -t.mean(), float(t.detach().abs().mean())
        out["expand"] = out["loss_1"] + out["loss_2"] + out["loss_3"]
        mag["expand"] = mag["loss_1"] + mag["loss_2"] + mag["loss_3"]
        out["norm"] = out["seed"] + out["expand"] + out["constrain"]
        mag["norm"] = mag["seed"] + mag["expand"] + mag["constrain"]
        out["seed_bg"] = out["seed_fg"] = torch.zeros((), dtype=torch.float64)
        mag["seed_bg"] = mag["seed_fg"] = 0.0
    elif method == "DSRG":
        for name, sl in (("seed_bg", slice(0, 1)), ("seed_fg", slice(1, None))):
            count = cues[..., sl].sum(dim=(1, 2, 3)) + 1e-8
            t = cues[..., sl] * torch.log(p[..., sl])
            out[name] = -(t.sum(dim=(1, 2, 3)) / count).mean()
            mag[name] = float((t.detach().abs().sum(dim=(1, 2, 3)) / count).mean())
        out["seed"], mag["seed"] = out["seed_bg"] + out["seed_fg"], mag["seed_bg"] + mag["seed_fg"]
        t = q * torch.log(q / (p + 1e-8) + 1e-8)
        out["constrain"] = t.sum() / (B * n)
        mag["constrain"] = float(t.detach().abs().sum() / (B * n))
        out["norm"], mag["norm"] = out["seed"] + out["constrain"], mag["seed"] + mag["constrain"]
        for k in ("expand", "loss_1", "loss_2", "loss_3"):
            out[k], mag[k] = torch.zeros((), dtype=torch.float64), 0.0
    else:
        raise ValueError(method)
    return out, mag


def stable_ranks(maps):
    """maps (B, n, C) numpy -> int ranks (B, n, C): ascending, among equal values the lower pixel index first"""
    order = np.argsort(maps, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(maps.shape[1])[None, :, None], maps.shape).copy(), axis=1)
    return rank


def rank_term_grads(p_np, labels_np):
    """d loss_1 / d p and d loss_3 / d p, float64 (B, h, w, C), the rank weights placed by stable argsort"""
    B, h, w, C = p_np.shape
    n = h * w
    maps = p_np.reshape(B, n, C).astype(np.float64)
    (w_fg, z_fg), (w_bg, z_bg) = ((w.astype(np.float64), float(z)) for w, z in (rank_weights(n, Q_FG), rank_weights(n, Q_BG)))
    rank = stable_ranks(p_np.reshape(B, n, C))
    srt = np.sort(maps, axis=1)
    mean_fg = (srt[:, :, 1:] * w_fg[None, :, None]).sum(1) / z_fg
    mean_bg = (srt[:, :, 0] * w_bg[None, :]).sum(1) / z_bg
    stat = (labels_np.reshape(B, C)[:, 1:] > 0).astype(np.float64)
    coeff = stat / np.maximum(stat.sum(1, keepdims=True), 1e-5)
    g1 = np.zeros((B, n, C))
    g1[:, :, 1:] = -(1.0 / B) * coeff[:, None, :] * (w_fg[rank[:, :, 1:]] / z_fg) / mean_fg[:, None, :]
    g3 = np.zeros((B, n, C))
    g3[:, :, 0] = -(1.0 / B) * (w_bg[rank[:, :, 0]] / z_bg) / mean_bg[:, None]
    return g1.reshape(p_np.shape), g3.reshape(p_np.shape)


def evaluate(method, prob, crf, cues, labels=None, min_prob=1e-4):
    """numpy float32 inputs -> (losses {name: float}, magnitudes {name: float}, g_p, g_z, parts {term: d term / d p}), float64.
    g_p is the sum of the parts: autograd for seed, constrain and loss_2, rank_term_grads for loss_1 and loss_3."""
    m = float(np.float32(min_prob))
    p = t64(prob).requires_grad_(True)
    lab = None if labels is None else t64(labels)
    out, mag = terms(method, p, t64(crf), t64(cues), lab)
    parts = {}
    for name in (("seed", "constrain", "loss_2") if method == "SEC" else ("seed", "constrain")):
        parts[name] = torch.autograd.grad(out[name], p, retain_graph=True)[0].numpy().copy()
    if method == "SEC":
        parts["loss_1"], parts["loss_3"] = rank_term_grads(np.asarray(prob), np.asarray(labels))
    g_p = sum(parts.values())
    g_z = grad_fc8(np.asarray(prob, dtype=np.float64), g_p, m)
    return {k: float(out[k].detach()) for k in KEYS}, mag, g_p, g_z, parts


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
def softmax_maps(rng, shape):
    """as tests/test_gpu_seg_chain.py::_softmax_maps"""
    e = np.exp(rng.normal(0, 2, shape))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def break_ties(prob):
    """Nudges equal values inside an (image, class) map apart by float32 steps, in place: the random cases carry no ties, so the tie
    rule cannot hide behind a tolerance (8192 float32 draws from (0, 1) do collide)."""
    B, h, w, C = prob.shape
    maps = prob.reshape(B, h * w, C)
    for b in range(B):
        for c in range(C):
            v = maps[b, :, c]
            while True:
                order = np.argsort(v, kind="stable")
                s = v[order]
                dup = np.nonzero(s[1:] == s[:-1])[0] + 1
                if not dup.size:
                    break
                v[order[dup]] = np.nextafter(s[dup], np.float32(np.inf))
    return prob


def has_ties(prob):
    B, h, w, C = prob.shape
    s = np.sort(prob.reshape(B, h * w, C), axis=1)
    return bool((s[:, 1:] == s[:, :-1]).any())


def make_case(shape, seed=0):
    """(B, H, W, C) -> prob, crf, cues, labels (float32), the inputs of the issue's cases: tie-free softmax maps; CRF
    log-probabilities (another softmax draw, clamped at 1e-4 and renormalised as the CRF layer's tail does); cues at density 0.2
    with image 1 (where there is one) without any cue; labels: image 0 all-positive (sum (1 - stat) = 0), the last image (B >= 2)
    background only, the others random.  B = 1: the single image is all-positive at an odd H * W, background only at an even one."""
    B, H, W, C = shape
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * C + H * W)
    prob = break_ties(softmax_maps(rng, shape))
    q = np.maximum(softmax_maps(rng, shape), np.float32(1e-4))
    crf = np.log(q / q.sum(-1, keepdims=True)).astype(np.float32)
    cues = (rng.random(shape) < 0.2).astype(np.float32)
    labels = (rng.random((B, C)) < 0.5).astype(np.float32)
    labels[:, 0] = 1.0
    labels[0, 1:] = 1.0
    if B >= 2:
        cues[1] = 0.0
        labels[B - 1, 1:] = 0.0
    elif (H * W) % 2 == 0:
        labels[0, 1:] = 0.0
    return prob, crf, cues, labels
