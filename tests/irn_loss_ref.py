"""Float64 oracle of the IRNet training loss (wsc_irn_aff_loss), in two independent forms.

  tensor_form   what the reference computes, restated: the path pixels gathered per path length, max-pooled along the path,
                1 - sigmoid, the two logs; the pair displacements from shifted slices of the field; the pair labels from the
                source / destination index tables; the batch reductions of the training step.  torch float64 with autograd, so
                it also gives d total / d edge and d total / d dp.  `sigmoid_first=True` is the reference's order (sigmoid, then
                the path maximum); the default takes the maximum on the logits, as the device does.
  pair_loop     a plain loop over (image, source, direction): labels, the path maximum, the terms, math.fsum.  Losses and counts
                only; small maps only.

Every input reaches the arithmetic as a float64 copy of a float32 value.  tests/test_reference_pins.py holds tensor_form(sigmoid_first=True)
and pair_labels to the per-pair tensors of the reference's own AffinityDisplacementLoss and GetAffinityLabelFromIndices
(tests/golden/ref_irn_loss.npz; regenerate with `python oracle/gen_golden_ref.py irn_loss`)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from wsscam.misc.indexing import PathIndex

KEYS = ("pos_bg", "pos_fg", "pos", "neg", "dp_fg", "dp_bg", "total", "n_bg", "n_fg", "n_neg")
LABEL_VALUES = np.array([0, 0, 3, 7, 255], np.uint8)
# (radius, B, h, w)
CASES = [(2, 1, 2, 3), (3, 2, 9, 11), (5, 2, 16, 20), (5, 3, 33, 37), (10, 1, 32, 40), (10, 1, 128, 128)]


def block_labels(rng, B, h, w, values=LABEL_VALUES, block=4):
    """(B, h, w) uint8: 4 x 4 blocks drawn from `values`"""
    hb, wb = (h + block - 1) // block, (w + block - 1) // block
    coarse = values[rng.integers(0, len(values), (B, hb, wb))]
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, axis=1), block, axis=2)[:, :h, :w])


def make_case(case, integer=False):
    """-> (edge float32 (B, h, w), dp float32 (B, 2, h, w), label uint8 (B, h, w)); integer: small integer values, so that path
    maxima tie and pair displacements hit 0 and their target"""
    radius, B, h, w = case
    rng = np.random.default_rng(1000 * radius + 100 * B + h + w + (7 if integer else 0))
    if integer:
        edge = rng.integers(-3, 4, (B, h, w)).astype(np.float32)
        dp = rng.integers(-2, 3, (B, 2, h, w)).astype(np.float32)
    else:
        edge = (2.0 * rng.standard_normal((B, h, w))).astype(np.float32)
        dp = (3.0 * rng.standard_normal((B, 2, h, w))).astype(np.float32)
    return edge, dp, block_labels(rng, B, h, w)


def pair_labels(label, pi, valid_below=21):
    """bg, fg, neg as bool (B, D, S): the reference's rule on the source / destination index tables"""
    flat = label.reshape(label.shape[0], -1)
    frm = flat[:, pi.src_indices][:, None, :]
    to = flat[:, pi.dst_indices]
    valid = np.logical_and(frm < valid_below, to < valid_below)
    equal = frm == to
    pos = np.logical_and(equal, valid)
    return np.logical_and(pos, frm == 0), np.logical_and(pos, frm > 0), np.logical_and(np.logical_not(equal), valid)


def tensor_form(edge, dp, label, radius, valid_below=21, sigmoid_first=False, grad=True):
    """-> dict: 'loss' {KEYS}, 'mag' {KEYS: sum of |terms| behind the value, scaled like it}, 'terms' {KEYS: number of terms},
    'g_edge' (B, h, w) and 'g_dp' (B, 2, h, w) float64 (grad=True), 'tied' the share of valid pairs whose path maximum is held
    by more than one pixel"""
    edge, dp = np.asarray(edge, np.float64), np.asarray(dp, np.float64)
    B, h, w = edge.shape
    pi = PathIndex(radius, default_size=(h, w))
    rf = pi.radius_floor
    e = torch.tensor(edge, requires_grad=grad)
    d = torch.tensor(dp, requires_grad=grad)
    bg_np, fg_np, neg_np = pair_labels(label, pi, valid_below)
    bg, fg, neg = (torch.from_numpy(a.astype(np.float64)) for a in (bg_np, fg_np, neg_np))
    # the affinity of every pair
    x = (torch.sigmoid(e) if sigmoid_first else e).view(B, -1)
    affs, tied = [], []
    for ind in pi.path_indices:  # (paths of this length, length, sources)
        dist = torch.index_select(x, 1, torch.from_numpy(ind).reshape(-1)).view(B, *ind.shape)
        m = F.max_pool2d(dist, (ind.shape[1], 1))
        tied.append(((dist == m).sum(dim=2) > 1).numpy())
        m = m.squeeze(2)
        affs.append(1 - (m if sigmoid_first else torch.sigmoid(m)))
    aff = torch.cat(affs, dim=1)  # (B, D, S)
    pos_term = -torch.log(aff + 1e-5)
    neg_term = -torch.log(1. + 1e-5 - aff)
    # the displacement of every pair
    ch, cw = h - rf, w - 2 * rf
    src = d[:, :, :ch, rf:rf + cw]
    dst = torch.stack([d[:, :, dy:dy + ch, rf + dx:rf + dx + cw] for dy, dx in pi.search_dst], 2)
    pair = (src.unsqueeze(2) - dst).reshape(B, 2, len(pi.search_dst), -1)
    target = torch.from_numpy(np.asarray(pi.search_dst, np.float64).T.copy()).view(1, 2, -1, 1)
    fg_dp = torch.abs(pair - target)
    bg_dp = torch.abs(pair)
    n_bg, n_fg, n_neg = bg.sum(), fg.sum(), neg.sum()
    sums = {"pos_bg": (bg * pos_term, n_bg + 1e-5), "pos_fg": (fg * pos_term, n_fg + 1e-5), "neg": (neg * neg_term, n_neg + 1e-5),
            "dp_fg": (fg_dp * fg.unsqueeze(1), 2 * n_fg + 1e-5), "dp_bg": (bg_dp * bg.unsqueeze(1), 2 * n_bg + 1e-5)}
    val = {k: t.sum() / den for k, (t, den) in sums.items()}
    mag = {k: float(t.detach().abs().sum() / den) for k, (t, den) in sums.items()}
    terms = {"pos_bg": int(n_bg), "pos_fg": int(n_fg), "neg": int(n_neg), "dp_fg": 2 * int(n_fg), "dp_bg": 2 * int(n_bg)}
    val["pos"] = val["pos_bg"] / 2 + val["pos_fg"] / 2
    val["total"] = (val["pos"] + val["neg"]) / 2 + (val["dp_fg"] + val["dp_bg"]) / 2
    mag["pos"] = mag["pos_bg"] / 2 + mag["pos_fg"] / 2
    mag["total"] = (mag["pos"] + mag["neg"]) / 2 + (mag["dp_fg"] + mag["dp_bg"]) / 2
    terms["pos"] = terms["pos_bg"] + terms["pos_fg"]
    terms["total"] = terms["pos"] + terms["neg"] + terms["dp_fg"] + terms["dp_bg"]
    out = {"mag": mag, "terms": terms}
    if grad:
        val["total"].backward()
        out["g_edge"], out["g_dp"] = e.grad.numpy().copy(), d.grad.numpy().copy()
    loss = {k: float(v.detach()) for k, v in val.items()}
    for k, n in (("n_bg", n_bg), ("n_fg", n_fg), ("n_neg", n_neg)):
        loss[k] = float(n)
        mag[k] = 0.0
        terms[k] = 0
    out["loss"] = loss
    valid = np.logical_or(np.logical_or(bg_np, fg_np), neg_np)
    out["tied"] = float(np.concatenate(tied, axis=1)[valid].mean()) if valid.any() else 0.0
    return out


def pair_loop(edge, dp, label, radius, valid_below=21):
    """-> {KEYS}: the losses and counts by a loop over every (image, source, direction)"""
    edge, dp = np.asarray(edge, np.float64), np.asarray(dp, np.float64)
    B, h, w = edge.shape
    pi = PathIndex(radius)
    rf = pi.radius_floor
    dirs, start, yx = pi.device_tables()
    t = {"pos_bg": [], "pos_fg": [], "neg": [], "dp_fg": [], "dp_bg": []}
    for b in range(B):
        for y in range(h - rf):
            for x in range(rf, w - rf):
                ls = int(label[b, y, x])
                for k, (dy, dx) in enumerate(dirs.tolist()):
                    lt = int(label[b, y + dy, x + dx])
                    if ls >= valid_below or lt >= valid_below:
                        continue
                    m = max(edge[b, y + py, x + px] for py, px in yx[start[k]:start[k + 1]].tolist())
                    aff = 1.0 - 1.0 / (1.0 + math.exp(-m))
                    if ls != lt:
                        t["neg"].append(-math.log(1.0 + 1e-5 - aff))
                        continue
                    pd = [dp[b, c, y, x] - dp[b, c, y + dy, x + dx] for c in (0, 1)]
                    if ls == 0:
                        t["pos_bg"].append(-math.log(aff + 1e-5))
                        t["dp_bg"] += [abs(pd[0]), abs(pd[1])]
                    else:
                        t["pos_fg"].append(-math.log(aff + 1e-5))
                        t["dp_fg"] += [abs(pd[0] - dy), abs(pd[1] - dx)]
    n_bg, n_fg, n_neg = len(t["pos_bg"]), len(t["pos_fg"]), len(t["neg"])
    out = {"pos_bg": math.fsum(t["pos_bg"]) / (n_bg + 1e-5), "pos_fg": math.fsum(t["pos_fg"]) / (n_fg + 1e-5),
           "neg": math.fsum(t["neg"]) / (n_neg + 1e-5), "dp_fg": math.fsum(t["dp_fg"]) / (2 * n_fg + 1e-5),
           "dp_bg": math.fsum(t["dp_bg"]) / (2 * n_bg + 1e-5), "n_bg": float(n_bg), "n_fg": float(n_fg), "n_neg": float(n_neg)}
    out["pos"] = out["pos_bg"] / 2 + out["pos_fg"] / 2
    out["total"] = (out["pos"] + out["neg"]) / 2 + (out["dp_fg"] + out["dp_bg"]) / 2
    return out


def loss_bound(mag, terms):
    """the largest |device - oracle| a loss value may show: both sides work in double and differ by the order of their sums"""
    return max(1e-10, 4.0 * terms * 2.0 ** -53) * mag
