"""float64 numpy oracle of the classifier loss head and of the ROC thresholds (include/wsscam.h: wsc_cls_loss, wsc_roc_thresholds,
wsc_cls_threshold_counts; 01_train/demo.py:60-61, utilities.py:69-165).

A restatement of the header's formulas: float32 inputs promoted to float64, p and 1 - p both formed from exp(-|l|), the clip
bounds eps = float32(1e-7) and hi = float32(1) - eps promoted.  tests/test_cls_head_oracle.py holds the loss and its gradients to
torch.autograd and the curve rule to sklearn.metrics.roc_curve; tests/test_reference_pins.py holds roc_thresholds and threshold_counts to
what the reference's own functions returned (tests/golden/ref_roc.npz; regenerate with `python oracle/gen_golden_ref.py roc`)."""
import numpy as np

EPS = np.float64(np.float32(1e-7))
HI = np.float64(np.float32(1) - np.float32(1e-7))
LOSS_KEYS = ("loss", "mean_loss", "n_equal", "tp", "possible", "predicted")
NO_POSITIVE, NO_NEGATIVE = 1, 2


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def sigmoid_pair(l):
    """(sigmoid(l), sigmoid(-l)), neither through a cancellation"""
    e = np.exp(-np.abs(l))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(l >= 0, big, small), np.where(l >= 0, small, big)


def pool(feat, kind):
    """feat (B, n, F) float64 -> (pooled (B, F), ties (B, F): the positions that hold the maximum; n for the mean)"""
    B, n, F = feat.shape
    if kind == "max":
        x = feat + 0.0  # -0 counts as +0
        mx = x.max(axis=1)
        return mx, (x == mx[:, None, :]).sum(axis=1)
    return feat.sum(axis=1) / n, np.full((B, F), n)


def cls_loss(feat, kind, w, bias, target, sample_w=None):
    """-> dict: 'values' {LOSS_KEYS}, 'mag' {'loss', 'mean_loss'} (the sums of |terms| behind the two loss values), 'p' (B, C)
    float64, 'logit', 'g_feat' (B, n, F), 'g_w' (C, F), 'g_bias' (C,) float64"""
    feat, w, z = f64(feat), f64(w), f64(target)
    B, n, F = feat.shape
    C = w.shape[0]
    wts = np.ones(B) if sample_w is None else f64(sample_w)
    nz = float(np.count_nonzero(wts))
    pooled, ties = pool(feat, kind)
    logit = pooled @ w.T + (0.0 if bias is None else f64(bias))
    p, q = sigmoid_pair(logit)
    pc, qc = np.clip(p, EPS, HI), np.clip(q, 1.0 - HI, 1.0 - EPS)
    term = -(z * np.log(pc) + (1.0 - z) * np.log(qc))
    ell = term.sum(axis=1) / C
    rp = np.rint(p)  # half to even
    values = {"loss": float((wts * ell).sum() / nz), "mean_loss": float(ell.sum() / B), "n_equal": int((z == rp).sum()),
              "tp": int(np.nansum(np.rint(z * p))), "possible": int(np.rint(z).sum()), "predicted": int(np.nansum(rp))}
    # (nansum: a NaN score has no rounding, the counts then cover the other cells -- the losses and the gradients are what carries it)
    mag = {"loss": float((wts[:, None] * np.abs(term)).sum() / (C * nz)), "mean_loss": float(np.abs(term).sum() / (C * B))}
    g_l = np.where((p >= EPS) & (p <= HI), (wts / (C * nz))[:, None] * (p - z), 0.0) + 0.0  # (+0.0 under a zero weight as well)
    g_l = np.where(np.isnan(p), p, g_l)  # (the clip's mask is false for a NaN, but what it gates is the sigmoid's NaN derivative times 0)
    g_pooled = g_l @ w
    if kind == "max":
        at_max = (feat + 0.0) == pooled[:, None, :]
        g_feat = np.where(at_max, (g_pooled / ties)[:, None, :], 0.0)
    else:
        g_feat = np.broadcast_to((g_pooled / n)[:, None, :], feat.shape).copy()
    return {"values": values, "mag": mag, "p": p, "logit": logit, "g_feat": g_feat, "g_w": g_l.T @ pooled, "g_bias": g_l.sum(axis=0),
            "ties": ties}


def margins_ok(p, margin=1e-6):
    """every p at least `margin` away from 0.5 and from both clip bounds: no count or mask hides behind summation differences"""
    return bool((np.abs(p - 0.5) >= margin).all() and (np.abs(p - EPS) >= margin).all() and (np.abs(p - HI) >= margin).all())


def make_case(shape, kind, seed=0, with_bias=True, with_weights=True):
    """(B, n, F, C) -> feat, w, bias or None, target, sample_w or None (float32); logits of a few units, margins asserted"""
    B, n, F, C = shape
    rng = np.random.default_rng(1000 * seed + 7 * B + n + F + C)
    feat = rng.normal(0, 1, (B, n, F)).astype(np.float32)
    spread = 2.0 / np.sqrt(F) * (np.sqrt(n) if kind == "mean" else 0.5)
    w = (rng.normal(0, 1, (C, F)) * spread).astype(np.float32)
    bias = rng.normal(0, 0.5, C).astype(np.float32) if with_bias else None
    target = (rng.random((B, C)) < 0.4).astype(np.float32)
    sample_w = None
    if with_weights:
        sample_w = rng.uniform(0.25, 3.0, B).astype(np.float32)
        if B > 1:
            sample_w[B // 2] = 0.0  # drops out of the sum and of the divisor
    res = cls_loss(feat, kind, w, bias, target, sample_w)
    assert margins_ok(res["p"]), "make_case: a probability within 1e-6 of 0.5 or a clip bound"
    if kind == "max":
        assert (res["ties"] == 1).all()
    return feat, w, bias, target, sample_w


def keras_ratios(values, n_elems, eps=1e-7):
    """binary_accuracy and f1 from the counts, utilities.py:69-97"""
    recall = values["tp"] / (values["possible"] + eps)
    precision = values["tp"] / (values["predicted"] + eps)
    return values["n_equal"] / float(n_elems), 2 * ((precision * recall) / (precision + recall + eps))


# ---- ROC -------------------------------------------------------------------------------------------------------------------------
def roc_points(t, s):
    """One class: targets (N,) 0/1, scores (N,) float32 -> (fps, tps int64, thresholds float32) of roc_curve(drop_intermediate=True)"""
    s = np.asarray(s, np.float32) + np.float32(0)
    pos = (np.asarray(t) == 1).astype(np.int64)
    order = np.argsort(-s.astype(np.float64), kind="stable")
    s2, t2 = s[order], pos[order]
    idx = np.nonzero(np.r_[s2[1:] != s2[:-1], True])[0]  # the last sample of each group of equal scores
    tps = np.cumsum(t2)[idx]
    fps = 1 + idx - tps
    th = s2[idx]
    keep = np.ones(len(tps), bool)
    if len(tps) > 2:
        keep[1:-1] = ((fps[2:] - 2 * fps[1:-1] + fps[:-2]) != 0) | ((tps[2:] - 2 * tps[1:-1] + tps[:-2]) != 0)
    return np.r_[0, fps[keep]], np.r_[0, tps[keep]], np.r_[np.float32(np.inf), th[keep]].astype(np.float32)


def roc_thresholds(scores, targets):
    """(N, C) float32 each -> thresholds float32 (C,), status int32 (C,), n_points int32 (C,), fps, tps int32 (C, N + 1)"""
    scores, targets = np.asarray(scores, np.float32), np.asarray(targets, np.float32)
    N, C = scores.shape
    thr, status, n_points = np.zeros(C, np.float32), np.zeros(C, np.int32), np.zeros(C, np.int32)
    fps_all, tps_all = np.zeros((C, N + 1), np.int32), np.zeros((C, N + 1), np.int32)
    for c in range(C):
        fps, tps, th = roc_points(targets[:, c], scores[:, c])
        K = len(th)
        n_points[c] = K
        fps_all[c, :K], tps_all[c, :K] = fps, tps
        P, Nn = int(tps[-1]), int(fps[-1])
        if P == 0 or Nn == 0:
            thr[c] = np.inf
            status[c] = (NO_POSITIVE if P == 0 else 0) | (NO_NEGATIVE if Nn == 0 else 0)
            continue
        tpr, fpr = tps / np.float64(P), fps / np.float64(Nn)
        thr[c] = th[np.argmin(np.abs(tpr - (1 - fpr)))]
    return thr, status, n_points, fps_all, tps_all


def threshold_counts(scores, targets, thr):
    """-> int64 (C, 5): TP, FP, TN, FN, #{target == (score >= thr)} (utilities.py:121-137)"""
    scores, targets = np.asarray(scores, np.float32), np.asarray(targets, np.float32)
    pred = scores >= np.asarray(thr, np.float32)[None, :]
    return np.stack([((targets == 1) & pred).sum(0), ((targets == 0) & pred).sum(0), ((targets == 0) & ~pred).sum(0),
                     ((targets == 1) & ~pred).sum(0), (targets == pred).sum(0)], axis=1).astype(np.int64)


def make_scores(N, C, seed=0, grid=False, degenerate=True):
    """scores that correlate with the targets; grid: rounded to eighths (heavy ties).  degenerate (C >= 3): class 1 without positives,
    class 2 with all scores equal."""
    rng = np.random.default_rng(seed + 31 * N + C)
    targets = (rng.random((N, C)) < rng.uniform(0.1, 0.6, C)[None, :]).astype(np.float32)
    scores = (0.6 * rng.random((N, C)) + 0.4 * targets * rng.random((N, C))).astype(np.float32)
    if grid:
        scores = (np.round(scores * 8) / 8).astype(np.float32)
    if degenerate and C >= 3:
        targets[:, 1] = 0.0
        scores[:, 2] = np.float32(0.375)
    return scores, targets
