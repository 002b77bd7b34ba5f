"""numpy oracle of the SEC / DSRG prediction tail (03a_sec-dsrg/model.py:665-719), used by tests/test_seg_eval_oracle.py and
tests/test_gpu_seg_eval.py.

    count_loop          model.py:698-719 restated literally over given label maps (the np.argmax of pred_curr) and ground truths:
                        bincount, masks, the gt_mask | pred_mask union -- the index form (VOC, :698-707) and the colour form
                        (ADP / DeepGlobe, :708-719)
    finish              :736-738
    resize_f64          the float64 half-pixel, clamped bilinear resize of an (h, w, C) map (the arithmetic oracle/hsn_ref.py
                        uses for cv2.resize INTER_LINEAR; restated here)
and the input generators both suites share."""
import numpy as np

# (h, w) -> (H, W): two upsizes (odd sizes, more than one block of 256 pixels), a downsize, the identity, one source pixel
SIZES = (((21, 27), (47, 61)), ((33, 33), (50, 37)), ((40, 40), (25, 31)), ((17, 19), (17, 19)), ((1, 1), (5, 4)))


def count_loop(labels, gts, num_classes, colours=None):
    """labels: list of (H, W) integer arg-max maps; gts: list of (H, W, 3) ground truths -- channel 0 the class index when
    colours is None (`gt_curr[:, :, 0] == k`), else colour-coded.  -> the five accumulators, float64 as the reference's."""
    intersect = np.zeros((num_classes))
    union = np.zeros((num_classes))
    confusion_matrix = np.zeros((num_classes, num_classes))
    gt_count = np.zeros((num_classes))
    pred_count = np.zeros((num_classes))
    for am, gt_curr in zip(labels, gts):
        am = np.asarray(am).astype(np.int64)
        pred_count += np.bincount(am.ravel(), minlength=num_classes)
        if colours is None:
            for k in range(num_classes):
                gt_mask = gt_curr[:, :, 0] == k
                pred_mask = am == k
                confusion_matrix[k, :] += np.bincount(am[gt_mask], minlength=num_classes)
                gt_count[k] += np.sum(gt_mask)
                intersect[k] += np.sum(gt_mask & pred_mask)
                union[k] += np.sum(gt_mask | pred_mask)
        else:
            gt_r = gt_curr[:, :, 0]
            gt_g = gt_curr[:, :, 1]
            gt_b = gt_curr[:, :, 2]
            for k, gt_colour in enumerate(colours):
                gt_mask = (gt_r == gt_colour[0]) & (gt_g == gt_colour[1]) & (gt_b == gt_colour[2])
                pred_mask = am == k
                confusion_matrix[k, :] += np.bincount(am[gt_mask], minlength=num_classes)
                gt_count[k] += np.sum(gt_mask)
                intersect[k] += np.sum(gt_mask & pred_mask)
                union[k] += np.sum(gt_mask | pred_mask)
    return {"intersect": intersect, "union": union, "confusion_matrix": confusion_matrix, "gt_count": gt_count,
            "pred_count": pred_count}


def finish(acc):
    """model.py:736-738 (and the IoU column of :740) on count_loop's accumulators."""
    out = dict(acc)
    out["IoU"] = acc["intersect"] / (acc["union"] + 1e-7)
    out["mIoU"] = np.mean(acc["intersect"] / (acc["union"] + 1e-7))
    out["precision"] = acc["intersect"] / (acc["gt_count"] + 1e-5)
    out["recall"] = acc["intersect"] / (acc["pred_count"] + 1e-5)
    return out


KEYS = ("intersect", "union", "confusion_matrix", "gt_count", "pred_count", "IoU", "mIoU", "precision", "recall")


def assert_metrics_equal(got, want):
    """Integers, then equal floats: every entry of `want` is in `got` with the same bits."""
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)), (k, got[k], want[k])


def resize_f64(m, out_hw):
    """(h, w, C) -> (H, W, C) in float64: src = (dst + 0.5) * in / out - 0.5 clamped to [0, in - 1], the two neighbours, linear."""
    m = np.asarray(m, dtype=np.float64)
    H, W = m.shape[:2]
    oh, ow = out_hw
    ys = np.clip((np.arange(oh) + 0.5) * H / oh - 0.5, 0, H - 1)
    xs = np.clip((np.arange(ow) + 0.5) * W / ow - 0.5, 0, W - 1)
    y0 = np.floor(ys).astype(int)
    x0 = np.floor(xs).astype(int)
    y1 = np.minimum(y0 + 1, H - 1)
    x1 = np.minimum(x0 + 1, W - 1)
    wy = (ys - y0)[:, None, None]
    wx = (xs - x0)[None, :, None]
    return (m[y0][:, x0] * (1 - wx) + m[y0][:, x1] * wx) * (1 - wy) + (m[y1][:, x0] * (1 - wx) + m[y1][:, x1] * wx) * wy


# ---- inputs -----------------------------------------------------------------------------------------------------------
def colours_for(num_classes):
    """Distinct RGB triples, one per class; (7, 7, 7) is none of them (the unlisted colour of the tests)."""
    return [(10 + 9 * k, 250 - 7 * k, (40 * k) % 256) for k in range(num_classes)]


UNLISTED = (7, 7, 7)


def make_gt_index(rng, H, W, num_classes, absent, border=True):
    """(H, W) uint8 class indices in blobs, class `absent` never occurs, a 255 frame (the VOC border) and a 255 speck."""
    yy, xx = np.mgrid[0:H, 0:W]
    score = rng.normal(0, 1, (num_classes, H, W))
    for k in range(num_classes):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.2, 0.5) * max(min(H, W), 2)
        score[k] += 4 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    score[absent] = -np.inf
    g = np.argmax(score, 0).astype(np.uint8)
    if border:
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 255
        g[H // 2, W // 2] = 255
    return g


def gt_as_image(g, colours=None):
    """The (H, W, 3) array the reference reads: the index in every channel (a palette PNG read as colour), or colour-coded with
    UNLISTED where the index is no class."""
    if colours is None:
        return np.repeat(g[:, :, None], 3, axis=2)
    out = np.empty(g.shape + (3,), np.uint8)
    out[:] = np.asarray(UNLISTED, np.uint8)
    for k, c in enumerate(colours):
        out[g == k] = np.asarray(c, np.uint8)
    return out


def make_labels(rng, H, W, num_classes, absent):
    """(H, W) int64 predictions from a draw unrelated to the ground truth; class `absent` is never predicted."""
    return make_gt_index(rng, H, W, num_classes, absent, border=False).astype(np.int64)
