"""03a_sec-dsrg mirror: the two host `py_func`s its training graph calls on every step, on libwsscam.

    generate_seed_step   DSRG.py:356-369 (and single_generate_seed_step :7-62 behind its process pool)
    crf_layer            the `crf` closure of DSRG.py:323-332 / SEC.py:270-280

The TF graph and the training of SEC / DSRG are out of scope; a DSRG model binds these two in place of the
closures it hands to tf.py_func and needs neither the process pool nor pydensecrf."""
import numpy as np

from . import _lib
from .misc.imutils import default_context


def generate_seed_step(tags, cues, probs, ctx=None, th_f=0.5, th_b=0.7):
    """DSRG seeded region growing of a batch (wsc_dsrg_seed_grow): one upload, one call, one download.

    tags  (B, C) or (B, 1, 1, C) float 0/1 image-level labels, class 0 = background
    cues  (B, H, W, C) float 0/1 seed cues
    probs (B, H, W, C) softmax
    -> float32 (B, H, W, C): the cues after growing.

    Returns a NEW array and leaves its inputs unmodified.  The reference mutates `cues` through a view (`cue[x, y, c] = 1`
    on `cues[i]`, DSRG.py:61) and returns the concatenation of those views' copies; a caller that relied on the side effect
    assigns the result back."""
    ctx = ctx or default_context()
    cues_f = np.ascontiguousarray(cues, dtype=np.float32)
    probs_f = np.ascontiguousarray(probs, dtype=np.float32)
    if cues_f.ndim != 4 or probs_f.shape != cues_f.shape:
        raise ValueError("generate_seed_step: cues %r and probs %r must both be (B, H, W, C)" % (np.shape(cues), np.shape(probs)))
    B, H, W, C = cues_f.shape
    tags_f = np.ascontiguousarray(tags, dtype=np.float32)
    if tags_f.shape not in ((B, C), (B, 1, 1, C)):
        raise ValueError("generate_seed_step: tags %r must be (B, C) or (B, 1, 1, C) for cues %r" % (tags_f.shape, cues_f.shape))
    # one buffer [tags | cues | probs]: one copy in, grown in place, one copy out
    n = cues_f.size
    packed = np.concatenate([tags_f.reshape(-1), cues_f.reshape(-1), probs_f.reshape(-1)])
    buf = ctx.to_device(packed, pooled=True)
    try:
        cues_dev = buf.ptr + 4 * tags_f.size
        _lib.dsrg_seed_grow(ctx, buf.ptr, cues_dev, cues_dev + 4 * n, B, H, W, C, cues_dev, th_f=th_f, th_b=th_b)
        return ctx.to_host(cues_dev, (B, H, W, C), np.float32)
    finally:
        buf.free()


def crf_layer(featmap, image, crf_config, num_classes, min_prob=1e-4, ctx=None, return_q=False):
    """The dense-CRF layer of SEC / DSRG: lib.crf.crf_inference(image[i], crf_config, num_classes, featmap[i],
    use_log=True) for every image of the batch, then clamp at min_prob, renormalise over classes and take the log.

    featmap (B, H, W, C) softmax at the seed size;  image (B, H, W, 3), cast to uint8 as the reference does.
    ONE wsc_crf over the B images and one mean-field loop (the reference builds B CRFs, one per image).
    -> float32 (B, H, W, C) log-probabilities; with return_q also the marginals (B, H, W, C) before that tail."""
    ctx = ctx or default_context()
    fm = np.asarray(featmap, dtype=np.float32)
    B, H, W, C = fm.shape
    if C != num_classes:
        raise ValueError("crf_layer: featmap has %d classes, num_classes = %d" % (C, num_classes))
    img = np.ascontiguousarray(np.asarray(image).astype(np.uint8))
    if img.shape != (B, H, W, 3):
        raise ValueError("crf_layer: image %r must be (B, H, W, 3) at the featmap's size %r" % (img.shape, fm.shape))
    U = np.ascontiguousarray(np.transpose(-np.log(fm), (0, 3, 1, 2)))  # [B][C][H*W]
    rgb_dev = ctx.to_device(img, pooled=True)
    u_dev = ctx.to_device(U, pooled=True)
    q_dev = ctx.alloc(U.nbytes, pooled=True)
    crf = _lib.Crf(ctx, rgb_dev, B, H, W, crf_config["g_sxy"], crf_config["bi_sxy"], crf_config["bi_srgb"])
    try:
        crf.inference(u_dev, C, crf_config["g_compat"], crf_config["bi_compat"], int(crf_config["iterations"]), q_dev, None)
        q = np.ascontiguousarray(np.transpose(ctx.to_host(q_dev, (B, C, H, W), np.float32), (0, 2, 3, 1)))
    finally:
        crf.close()
        for d in (rgb_dev, u_dev, q_dev):
            d.free()
    ret = q.copy()
    ret[ret < min_prob] = min_prob
    ret /= np.sum(ret, axis=3, keepdims=True)
    ret = np.log(ret).astype(np.float32)
    return (ret, q) if return_q else ret


# ---- the prediction tail: eval_miou with is_eval=True (model.py:665-719, called from predict :542-586) -------------------------
def seg_gt_index(gt, num_classes, colours=None):
    """Ground truth of one image -> uint8 class index plane (H, W) in [0, num_classes].

    colours=None: `gt` is the class-index plane (H, W), or the (H, W, k) image whose channel 0 holds it -- the reference's VOC
    test is `gt[:, :, 0] == k` (model.py:701).  colours set: `gt` is (H, W, 3) colour-coded, the ADP / DeepGlobe test of
    :713-714 (hsn.demo.gt_index_from_colours).  A pixel that matches no class -- the VOC 255 border, an unlisted colour -- gets
    the extra index num_classes: it is in no ground-truth mask but still counts in pred_count and, through the prediction
    masks, in the unions."""
    if colours is not None:
        from .hsn.demo import gt_index_from_colours

        if len(colours) != num_classes:
            raise ValueError("seg_gt_index: %d colours for %d classes" % (len(colours), num_classes))
        return gt_index_from_colours(gt, colours)
    g = np.asarray(gt)
    if g.ndim == 3:
        g = g[:, :, 0]
    if g.ndim != 2:
        raise ValueError("seg_gt_index: ground truth %r must be (H, W) or (H, W, k)" % (np.shape(gt),))
    return np.where((g >= 0) & (g < num_classes), g, num_classes).astype(np.uint8)


def seg_metrics_from_confusion(conf):
    """The numbers of model.py:698-719 and :736-738 from the (C+1) x (C+1) matrix conf[gt][pred] whose extra row holds the
    pixels of no class (the extra column stays empty: an arg-max is a class).  float64 throughout, as the reference's
    accumulators are; `precision` and `recall` carry the reference's names, which are swapped relative to the usual ones."""
    conf = np.asarray(conf)
    n = conf.shape[0] - 1
    assert conf.shape == (n + 1, n + 1) and n >= 1, conf.shape
    intersect = np.diag(conf)[:n].astype(np.float64)
    gt_count = conf[:n, :].sum(1).astype(np.float64)
    pred_count = conf[:, :n].sum(0).astype(np.float64)  # np.bincount over every pixel, whatever its ground truth (:699)
    union = gt_count + pred_count - intersect  # np.sum(gt_mask | pred_mask) (:707)
    iou = intersect / (union + 1e-7)
    return {"intersect": intersect, "union": union, "gt_count": gt_count, "pred_count": pred_count,
            "confusion_matrix": conf[:n, :n].astype(np.float64), "IoU": iou, "mIoU": float(np.mean(iou)),
            "precision": intersect / (gt_count + 1e-5), "recall": intersect / (pred_count + 1e-5)}


class SegEvaluator:
    """The per-image loop of eval_miou (model.py:665-719, is_eval=True) for a batch at a time, device resident between the
    upload of the network's softmax maps and the confusion matrix.

    resize_after_crf=False (VOC, ADP; :686-689): image and map are brought to the ground truth's size, CRF there.
    resize_after_crf=True (DeepGlobe; :693-695): CRF at the network size on the image as given, the marginals are resized.
    crf_config: {g_sxy, g_compat, bi_sxy, bi_srgb, bi_compat, iterations} (model.crf_config_test).
    The matrix stays on the device over the whole run; metrics() downloads it."""

    def __init__(self, num_classes, crf_config, colours=None, resize_after_crf=False, ctx=None):
        self.ctx = ctx or default_context()
        self.C = int(num_classes)
        if not 1 <= self.C <= 32:
            raise ValueError("SegEvaluator: num_classes = %d (the dense CRF takes 1..32 classes)" % self.C)
        self.cfg = dict(crf_config)
        self.colours = None if colours is None else [tuple(int(v) for v in c) for c in colours]
        if self.colours is not None and len(self.colours) != self.C:
            raise ValueError("SegEvaluator: %d colours for %d classes" % (len(self.colours), self.C))
        self.resize_after_crf = bool(resize_after_crf)
        nbytes = (self.C + 1) * (self.C + 1) * 8
        self.conf_dev = self.ctx.alloc(nbytes, pooled=True)
        _lib.check(self.ctx._lib.wsc_memset(self.ctx.h, self.conf_dev.ptr, 0, nbytes))

    def close(self):
        if getattr(self, "conf_dev", None) is not None:
            self.conf_dev.free()
            self.conf_dev = None

    def update(self, probs, images, gts, want_pred=False):
        """probs[b] (h_b, w_b, C) float32 softmax (> 0), images[b] (H, W, 3) uint8, gts[b] as seg_gt_index takes it.
        -> with want_pred the list of (H_b, W_b) uint8 label maps at the ground truths' sizes, else None."""
        ctx, C, cfg = self.ctx, self.C, self.cfg
        B = len(probs)
        if B == 0 or len(images) != B or len(gts) != B:
            raise ValueError("SegEvaluator.update: %d maps, %d images, %d ground truths" % (B, len(images), len(gts)))
        maps = [np.ascontiguousarray(p, dtype=np.float32) for p in probs]
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        gt = [np.ascontiguousarray(seg_gt_index(g, C, self.colours)) for g in gts]
        for b in range(B):
            if maps[b].ndim != 3 or maps[b].shape[2] != C or imgs[b].ndim != 3 or imgs[b].shape[2] != 3:
                raise ValueError("SegEvaluator.update: image %d: map %r must be (h, w, %d), image %r (H, W, 3)"
                                 % (b, maps[b].shape, C, imgs[b].shape))
            if self.resize_after_crf and imgs[b].shape[:2] != maps[b].shape[:2]:
                raise ValueError("SegEvaluator.update: image %d: with resize_after_crf the image %r has the map's size %r"
                                 % (b, imgs[b].shape[:2], maps[b].shape[:2]))
        src_hw = [m.shape[:2] for m in maps]
        out_hw = [g.shape for g in gt]
        crf_hw = src_hw if self.resize_after_crf else out_hw  # where the CRF runs
        n_out = [h * w for h, w in out_hw]
        n_crf = [h * w for h, w in crf_hw]
        prob_off = np.concatenate(([0], np.cumsum([m.size for m in maps])))
        crf_off = np.concatenate(([0], np.cumsum(n_crf)))  # pixels; times C: the unaries / marginals
        out_off = np.concatenate(([0], np.cumsum(n_out)))
        # one uint8 upload: [images that already have the CRF's size | images to resize | ground truths]; an image that is
        # resized lands in `res_dev`, the images of one target size next to each other (one wsc_resize_u8 per size)
        todo = {}
        for b in range(B):
            if imgs[b].shape[:2] != tuple(crf_hw[b]):  # (cv2.resize returns a copy otherwise)
                todo.setdefault(tuple(crf_hw[b]), []).append(b)
        rgb_at, res_at, src_at, parts, pos, res_bytes = [None] * B, [None] * B, [None] * B, [], 0, 0
        for b in range(B):
            if imgs[b].shape[:2] == tuple(crf_hw[b]):
                rgb_at[b] = pos
                parts.append(imgs[b].reshape(-1))
                pos += imgs[b].size
        for hw, bs in todo.items():
            for b in bs:
                src_at[b], res_at[b] = pos, res_bytes
                parts.append(imgs[b].reshape(-1))
                pos += imgs[b].size
                res_bytes += hw[0] * hw[1] * 3
        gt_at = pos
        parts.extend(g.reshape(-1) for g in gt)
        bufs = []

        def dev(buf):
            bufs.append(buf)
            return buf

        crf = None
        try:
            u8_dev = dev(ctx.to_device(np.concatenate(parts), pooled=True))
            prob_dev = dev(ctx.to_device(np.concatenate([m.reshape(-1) for m in maps]), pooled=True))
            rgb_ptr = [None if rgb_at[b] is None else u8_dev.ptr + rgb_at[b] for b in range(B)]
            if todo:
                res_dev = dev(ctx.alloc(res_bytes, pooled=True))
                for hw, bs in todo.items():
                    _lib.resize_u8(ctx, u8_dev, [imgs[b].shape[:2] for b in bs], [src_at[b] for b in bs], hw,
                                   res_dev.ptr + res_at[bs[0]])
                    for b in bs:
                        rgb_ptr[b] = res_dev.ptr + res_at[b]
            u_dev = dev(ctx.alloc(int(crf_off[-1]) * C * 4, pooled=True))
            _lib.seg_unary_nhwc(ctx, prob_dev, C, src_hw, crf_hw, prob_off[:-1], crf_off[:-1] * C, u_dev)
            lab_dev = dev(ctx.alloc(int(out_off[-1]) * 4, pooled=True))
            crf = _lib.CrfV(ctx, rgb_ptr, crf_hw, cfg["g_sxy"], cfg["bi_sxy"], cfg["bi_srgb"])
            u_ptr = [u_dev.ptr + int(crf_off[b]) * C * 4 for b in range(B)]
            if self.resize_after_crf:
                q_dev = dev(ctx.alloc(int(crf_off[-1]) * C * 4, pooled=True))
                crf.inference(u_ptr, [C] * B, cfg["g_compat"], cfg["bi_compat"], int(cfg["iterations"]),
                              q_ptrs=[q_dev.ptr + int(crf_off[b]) * C * 4 for b in range(B)])
                _lib.seg_resize_argmax(ctx, q_dev, C, src_hw, out_hw, crf_off[:-1] * C, out_off[:-1], lab_dev)
            else:
                crf.inference(u_ptr, [C] * B, cfg["g_compat"], cfg["bi_compat"], int(cfg["iterations"]),
                              argmax_ptrs=[lab_dev.ptr + int(out_off[b]) * 4 for b in range(B)])
            pred_dev = dev(ctx.alloc(int(out_off[-1]), pooled=True)) if want_pred else None
            # ignore_label -1: no uint8 ground-truth index equals it, every pixel is counted
            _lib.label_confusion_nn(ctx, lab_dev, out_hw, out_hw, out_off[:-1], u8_dev.ptr + gt_at, C + 1, self.conf_dev,
                                    pred_dev=pred_dev, ignore_label=-1)
            if want_pred:
                flat = ctx.to_host(pred_dev, (int(out_off[-1]),), np.uint8)
                return [flat[out_off[b]:out_off[b + 1]].reshape(out_hw[b]) for b in range(B)]
            return None
        finally:
            if crf is not None:
                crf.close()
            for d in bufs:
                d.free()

    def metrics(self):
        conf = self.ctx.to_host(self.conf_dev, (self.C + 1, self.C + 1), np.int64)
        return seg_metrics_from_confusion(conf)
