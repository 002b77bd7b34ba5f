"""03a_sec-dsrg mirror on libwsscam: the network's forward pass, the two host `py_func`s of its graph, the prediction tail.

    SegNet               the DeepLab-VGG16 forward pass of SEC.py:117-128 / DSRG.py:169-186 at drop_prob = 0: fc8-softmax,
                         create_network's output (the CRF layer) and pred()'s rescale_output; image_preprocess (model.py:335-340)
    generate_seed_step   DSRG.py:356-369 (and single_generate_seed_step :7-62 behind its process pool)
    crf_layer            the `crf` closure of DSRG.py:323-332 / SEC.py:270-280
    SegEvaluator         eval_miou (model.py:665-719)
    DeviceMaps           an array that stays on the device between those calls; SegNet's *_dev methods, crf_layer_dev and
                         SegEvaluator.update take and return it
    Predictor            Model.predict's loop (model.py:542-586): decoded images in, confusion matrix out, nothing in between
                         on the host
    SegLoss              getloss() (SEC.py:363-465, DSRG.py:459-518) and the gradient it sends into fc8 (wsc_seg_loss);
                         rank_weights forms SEC's rank-pooling tables; SegNet.loss_step_dev is the non-backward half of one
                         training step of Model.train at drop_prob = 0: forward, CRF layer, region growing, losses
    SegGrads             opt.compute_gradients (model.py:382-387) at drop_prob = 0: SegNet.forward_dev(keep=True) keeps the tape,
                         SegNet.backward_dev carries d loss / d fc8 to the gradient of every weight and bias, in exact fp32;
                         SegNet.grad_step_dev is loss_step_dev followed by it

    SegTrainer           Model.optimize() and the update branch of Model.train() (model.py:379-404, 491-504): at drop_prob = 0 the
                         reference's `debug` graph, at 0.5 its `train` phase (dropout behind fc6 / fc7): the weight decay term, the lr multipliers, gradient accumulation, the momentum
                         update and the write-back of the weights into the net (wsc_seg_sgd_accumulate / _apply,
                         wsc_net_seg_load_params); parameters, momentum and accumulator never leave the device

    SegBatcher           Model.next_batch (model.py:207-348): the inputs of a training step -- network input, dense cues from the
                         sparse lists of localization_cues.pickle (load_cues), labels -- and of a validation batch -- network input,
                         ground-truth class indices -- as DeviceMaps (wsc_seg_train_batch, wsc_seg_gt_index_tf), with numpy twins
    SegTrainLoop, train  Model.train() (model.py:435-540): shuffled_ids' order, one SegTrainer.step per iteration, the reports with
                         the validation mIoU of the is_eval=False pass, epoch-<i>.npy / final-0.npy, resume

Dropout (SegNet.forward_dev(dropout=...), SegTrainer(drop_prob=0.5)) has the project's own counter-based keep-masks, not
TensorFlow's random stream, and so has the shuffle order (shuffled_ids: numpy's generator); reading TensorFlow checkpoints is out of
scope.  Nothing here imports
TensorFlow: Model.predict runs on this module alone."""
import numpy as np

from . import _lib
from .device import DeviceMaps, Freed, device_input, device_operand  # noqa: F401  (DeviceMaps, Freed, device_operand: re-exported)
from .misc.imutils import default_context, prefetched
from .trainer import TrainerCore


class SegGrads(Freed):
    """The gradient of every weight and bias of a SegNet, on the device: one float32 DeviceMaps (`maps`) and the `layout`
    {layer: {'k', 'Cin', 'Cout', 'w_off', 'b_off'}} (offsets in floats).  grads[layer] downloads that layer as {'w': HWIO array,
    'b': [Cout] array}; .ptr(layer, 'w' | 'b') is the device address for a trainer that wraps the buffer; .to_host() every layer
    in one download; .free() / a context manager releases the buffer."""

    def __init__(self, maps, layout):
        self.maps = maps
        self.layout = layout

    def _shape(self, layer, which):
        e = self.layout[layer]
        return (e["k"], e["k"], e["Cin"], e["Cout"]) if which == "w" else (e["Cout"],)

    def ptr(self, layer, which):
        if which not in ("w", "b"):
            raise KeyError("SegGrads: %r is neither 'w' nor 'b'" % (which,))
        return self.maps.ptr + 4 * self.layout[layer][which + "_off"]

    def keys(self):
        return self.layout.keys()

    def __getitem__(self, layer):
        e = self.layout[layer]
        return {which: self.maps.ctx.to_host(self.maps.buf, self._shape(layer, which), np.float32, offset_bytes=4 * e[which + "_off"])
                for which in ("w", "b")}

    def to_host(self):
        return _lib.unflatten(self.maps.to_host(), _lib.SegGrad.fields(self.layout))


class SegTape(DeviceMaps):
    """The tape of SegNet.forward_dev(keep=True): a flat float32 DeviceMaps of `elems` floats with `entries` (the plan of
    wsc_net_seg_tape_plan), `input_shape` (B, H, W) and `drop_prob` (0.0: a forward pass without dropout)."""

    def __init__(self, ctx, elems, entries, input_shape, drop_prob=0.0):
        super().__init__(ctx, (elems,), np.float32)
        self.entries, self.input_shape, self.drop_prob = entries, tuple(input_shape), float(drop_prob)


def _image_blocks(images):
    """uint8 DeviceMaps -> ([(h, w)], byte offsets): a packed ragged batch, or (B, H, W, 3)."""
    if images.dtype != np.uint8:
        raise ValueError("device images must be uint8, got %s" % images.dtype)
    if images.sizes is not None:
        return [tuple(int(v) for v in hw) for hw in images.sizes], [int(o) for o in images.offsets]
    if len(images.shape) != 4 or images.shape[3] != 3:
        raise ValueError("device images %r must be (B, H, W, 3) or a packed ragged batch" % (images.shape,))
    B, H, W, _ = images.shape
    return [(H, W)] * B, [b * H * W * 3 for b in range(B)]


def _seed_hw(seed_size, map_hw):
    if seed_size is None:
        return tuple(map_hw)
    return (int(seed_size), int(seed_size)) if np.isscalar(seed_size) else (int(seed_size[0]), int(seed_size[1]))


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


def generate_seed_step_dev(tags, cues, probs, ctx=None, th_f=0.5, th_b=0.7):
    """generate_seed_step on device buffers: cues and probs are float32 DeviceMaps (B, H, W, C), tags a DeviceMaps (B, C) or a host
    array as generate_seed_step takes it (uploaded once) -> a NEW DeviceMaps (B, H, W, C) with the grown cues, generate_seed_step's
    bits (the same wsc_dsrg_seed_grow).  The inputs are not modified."""
    ctx = ctx or cues.ctx
    for name, a in (("cues", cues), ("probs", probs)):
        if not isinstance(a, DeviceMaps) or a.dtype != np.float32 or len(a.shape) != 4:
            raise ValueError("generate_seed_step_dev: %s must be a float32 DeviceMaps (B, H, W, C), got %r" % (name, getattr(a, "shape", type(a))))
    if probs.shape != cues.shape:
        raise ValueError("generate_seed_step_dev: cues %r and probs %r must both be (B, H, W, C)" % (cues.shape, probs.shape))
    B, H, W, C = cues.shape
    tags_dev = mine = None
    if isinstance(tags, DeviceMaps):
        if tags.dtype != np.float32 or tags.shape not in ((B, C), (B, 1, 1, C)):
            raise ValueError("generate_seed_step_dev: tags %r %s must be float32 (B, C) for cues %r" % (tags.shape, tags.dtype, cues.shape))
        tags_dev = tags
    else:
        tags_f = np.ascontiguousarray(tags, dtype=np.float32)
        if tags_f.shape not in ((B, C), (B, 1, 1, C)):
            raise ValueError("generate_seed_step_dev: tags %r must be (B, C) or (B, 1, 1, C) for cues %r" % (tags_f.shape, cues.shape))
        tags_dev = mine = DeviceMaps.from_host(ctx, tags_f)
    out = None
    try:
        out = DeviceMaps(ctx, cues.shape, np.float32)
        _lib.dsrg_seed_grow(ctx, tags_dev.ptr, cues.ptr, probs.ptr, B, H, W, C, out.ptr, th_f=th_f, th_b=th_b)
        return out
    except Exception:
        if out is not None:
            out.free()
        raise
    finally:
        if mine is not None:
            mine.free()


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


def crf_layer_dev(prob, x, img_mean, crf_config, num_classes, min_prob=1e-4, seed_size=None, ctx=None):
    """The whole build_crf layer (DSRG.py:302-335 / SEC.py:252-283) without a host copy.

    prob DeviceMaps (B, h, w, C) fc8-softmax;  x DeviceMaps (B, H, W, 3), the network's input;  img_mean (3,) in x's channel order.
    The image x + img_mean and -- when seed_size differs from (h, w) -- the map are brought to the seed size with the TF sampler
    (wsc_seg_crf_image_u8, wsc_resize_bilinear_tf), the unaries are -log of the map (wsc_seg_unary_nhwc at equal sizes: its
    pass-through), ONE wsc_crf runs over the B images, and wsc_seg_crf_logprob clamps, renormalises and takes the log.
    -> DeviceMaps float32 (B, s_h, s_w, C) log-probabilities.  Against crf_layer on SegNet.resize's image: the unaries use the
    device logf where crf_layer uses np.log, and the tail sums in class order in fp32."""
    ctx = ctx or prob.ctx
    if len(prob.shape) != 4 or prob.dtype != np.float32 or len(x.shape) != 4 or x.shape[3] != 3 or x.dtype != np.float32:
        raise ValueError("crf_layer_dev: prob %r must be float32 (B, h, w, C), x %r float32 (B, H, W, 3)" % (prob.shape, x.shape))
    B, h, w, C = prob.shape
    if C != num_classes:
        raise ValueError("crf_layer_dev: prob has %d classes, num_classes = %d" % (C, num_classes))
    if x.shape[0] != B:
        raise ValueError("crf_layer_dev: %d maps for %d images" % (B, x.shape[0]))
    sh, sw = _seed_hw(seed_size, (h, w))
    n = sh * sw
    bufs = [ctx.alloc(B * n * 3, pooled=True), ctx.alloc(B * n * C * 4, pooled=True), ctx.alloc(B * n * C * 4, pooled=True)]
    img_dev, u_dev, q_dev = bufs
    out = DeviceMaps(ctx, (B, sh, sw, C), np.float32)
    crf = None
    try:
        _lib.seg_crf_image_u8(ctx, x.ptr, B, x.shape[1], x.shape[2], img_mean, (sh, sw), img_dev)
        fmap = prob.ptr
        if (h, w) != (sh, sw):  # (the TF resize to the same size is the identity)
            bufs.append(ctx.alloc(B * n * C * 4, pooled=True))
            fmap = _lib.resize_bilinear_tf(ctx, prob.ptr, B, h, w, C, sh, sw, bufs[-1]).ptr
        off = np.arange(B, dtype=np.int64) * (n * C)
        _lib.seg_unary_nhwc(ctx, fmap, C, [(sh, sw)] * B, [(sh, sw)] * B, off, off, u_dev)
        crf = _lib.Crf(ctx, img_dev, B, sh, sw, crf_config["g_sxy"], crf_config["bi_sxy"], crf_config["bi_srgb"])
        crf.inference(u_dev, C, crf_config["g_compat"], crf_config["bi_compat"], int(crf_config["iterations"]), q_dev, None)
        _lib.seg_crf_logprob(ctx, q_dev, B, C, n, min_prob, out.ptr)
        return out
    except Exception:
        out.free()
        raise
    finally:
        if crf is not None:
            crf.close()
        for d in bufs:
            d.free()


# ---- the loss head: getloss() and d loss / d fc8 (SEC.py:363-465, DSRG.py:459-518) ---------------------------------------------
SEC_Q_FG, SEC_Q_BG = 0.996, 0.999  # get_expand_loss's decay rates (SEC.py:413,420)


def rank_weights(n, q):
    """The global-weighted-rank-pooling constants of get_expand_loss (SEC.py:415-418) as TensorFlow sees them:
    w64 = np.array([q ** i for i in range(n - 1, -1, -1)]) -> (float32(w64), float32(np.sum(w64)))."""
    w64 = np.array([q ** i for i in range(int(n) - 1, -1, -1)])
    return w64.astype(np.float32), np.float32(np.sum(w64))


class SegLoss:
    """getloss() of SEC / DSRG on the device, with the gradient of its value with respect to fc8-softmax or to the fc8 logits
    (wsc_seg_loss; the formulas, the tie rules and the double arithmetic: include/wsscam.h).  `crf` and the cues are constants to
    the gradient, as they are in the reference graph (both come out of tf.py_func).

    loss = SegLoss("SEC" | "DSRG", num_classes, min_prob=1e-4, ctx=None)
    losses, grad = loss(prob, crf, cues, labels=None, want_grad="fc8")
      prob, crf, cues  (B, h, w, C): fc8-softmax, the CRF layer's log-probabilities, the 0/1 cues (DSRG: the grown ones) -- float32
                       DeviceMaps, read in place, or host arrays, uploaded once
      labels           (B, C) or (B, 1, 1, C) image labels, class 0 = background: SEC's expand loss needs them; DSRG ignores them
      want_grad        "fc8": d norm / d fc8 (for DSRG the gradient of each of fc8_1 .. fc8_4);  "prob": d norm / d fc8-softmax;
                       None: losses only
      -> ({"seed", "constrain", "expand", "norm", "loss_1", "loss_2", "loss_3", "seed_bg", "seed_fg"} as Python floats -- the
          reference's self.loss keys and getloss's value under "norm", as Model.train logs it; a part the method lacks is 0.0 --,
          a new float32 DeviceMaps (B, h, w, C) or None)
    The call downloads the nine loss values and nothing else.  SEC's weight tables are cached per h * w."""

    def __init__(self, method, num_classes, min_prob=1e-4, ctx=None):
        if method not in ("SEC", "DSRG"):
            raise ValueError("SegLoss: method %r is neither 'SEC' nor 'DSRG'" % (method,))
        self.method = method
        self.C = int(num_classes)
        if not 2 <= self.C <= 32:
            raise ValueError("SegLoss: num_classes = %d (2 .. 32, class 0 is the background)" % self.C)
        self.min_prob = float(min_prob)
        self.ctx = ctx or default_context()
        self._weights = {}  # n -> (w_fg, z_fg, w_bg, z_bg)

    def weights(self, n):
        if n not in self._weights:
            self._weights[n] = rank_weights(n, SEC_Q_FG) + rank_weights(n, SEC_Q_BG)
        return self._weights[n]

    def _maps(self, name, a, shape, held):
        return device_operand(self, self.ctx, name, a, np.float32, shape, held)

    def __call__(self, prob, crf, cues, labels=None, want_grad="fc8"):
        if want_grad not in ("fc8", "prob", None):
            raise ValueError("SegLoss: want_grad %r is not 'fc8', 'prob' or None" % (want_grad,))
        sec = self.method == "SEC"
        if sec and labels is None:
            raise ValueError("SegLoss: labels is None: SEC's expand loss reads the image labels")
        ctx, held, grad = self.ctx, [], None
        try:
            p = self._maps("prob", prob, lambda s: len(s) == 4 and s[3] == self.C and 0 not in s, held)  # any (B, h, w, C)
            B, h, w, C = p.shape
            q = self._maps("crf", crf, p.shape, held)
            cu = self._maps("cues", cues, p.shape, held)
            lab = self._maps("labels", labels, lambda s: s in ((B, C), (B, 1, 1, C)), held) if sec else None
            w_fg, z_fg, w_bg, z_bg = self.weights(h * w) if sec else (None, 0.0, None, 0.0)
            loss_dev = DeviceMaps(ctx, (len(_lib.SEG_LOSS_SLOTS),), np.float64)
            held.append(loss_dev)
            if want_grad is not None:
                grad = DeviceMaps(ctx, p.shape, np.float32)
            _lib.seg_loss(ctx, _lib.SEG_LOSS_SEC if sec else _lib.SEG_LOSS_DSRG, p.ptr, q.ptr, cu.ptr, lab.ptr if sec else None, B, h, w,
                          C, self.min_prob, w_fg, z_fg, w_bg, z_bg, loss_dev.ptr,
                          grad_prob_dev=grad.ptr if want_grad == "prob" else None,
                          grad_fc8_dev=grad.ptr if want_grad == "fc8" else None)
            values = loss_dev.to_host()
            return {k: float(v) for k, v in zip(_lib.SEG_LOSS_SLOTS, values)}, grad
        except Exception:
            if grad is not None:
                grad.free()
            raise
        finally:
            for d in held:
                d.free()


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
    """The per-image loop of eval_miou (model.py:665-719) for a batch at a time, device resident between the network's softmax maps
    and the confusion matrix.

    resize_after_crf=False (VOC, ADP; :686-689): image and map are brought to the ground truth's size, CRF there.
    resize_after_crf=True (DeepGlobe; :693-695): CRF at the network size on the image as given, the marginals are resized.
    crf_config: {g_sxy, g_compat, bi_sxy, bi_srgb, bi_compat, iterations} (model.crf_config_test).
    crf=False: the is_eval=False pass (:666-669, :698-719) -- no resize and no CRF, the arg-max of the map as it is against a
    ground truth of the map's size; crf_config, resize_after_crf and update()'s images are not used.
    The matrix stays on the device over the whole run; metrics() downloads it.

    saveimg_dir (eval_miou's saveimg_dir with single_crf_metrics, model.py:596-612, the is_eval pass): update(..., ids=...) writes
    per image `<id>_img.png` (the image at the ground truth's size), `<id>_pred.png` (label2rgb of the arg-max) and
    `<id>_output.png` (should_overlay: np.uint8(0.25 * img + 0.75 * label2rgb), else the colour map again), the colour map and the
    overlay rendered on the device from the label maps the counting pass reads (wsc_render_labels).  quarter_size=True is the
    DeepGlobe branch (:597-600): image (cv2's 8-bit INTER_LINEAR) and map (nearest; a nearest resize of the marginals commutes
    with their arg-max) at `dsize=(shape[0] // 4, shape[1] // 4)`.  palette: the dataset's label2rgb_colors (:95-140), default
    `colours`.  model.label2rgb hands skimage's label2rgb `colors=label2rgb_colors[unique labels present]`; skimage cycles through
    that list in the order of the labels it finds, so label k gets label2rgb_colors[k]: a plain palette lookup for every label
    below category_num -- the only ones an arg-max over category_num channels gives.  (skimage is not installed where this package
    was developed: that reading of label2rgb is UNPINNED)"""

    def __init__(self, num_classes, crf_config, colours=None, resize_after_crf=False, ctx=None, crf=True, saveimg_dir=None,
                 should_overlay=False, quarter_size=False, palette=None):
        self.ctx = ctx or default_context()
        self.C = int(num_classes)
        if not 1 <= self.C <= 32:
            raise ValueError("SegEvaluator: num_classes = %d (the dense CRF takes 1..32 classes)" % self.C)
        self.cfg = dict(crf_config) if crf_config is not None else {}
        self.colours = None if colours is None else [tuple(int(v) for v in c) for c in colours]
        if self.colours is not None and len(self.colours) != self.C:
            raise ValueError("SegEvaluator: %d colours for %d classes" % (len(self.colours), self.C))
        self.resize_after_crf = bool(resize_after_crf)
        self.crf = bool(crf)
        self.saveimg_dir, self.should_overlay, self.quarter_size = saveimg_dir, bool(should_overlay), bool(quarter_size)
        self.palette = self.colours if palette is None else [tuple(int(v) for v in c) for c in palette]
        if saveimg_dir is not None and (self.palette is None or len(self.palette) != self.C):
            raise ValueError("SegEvaluator: saveimg_dir needs a palette of %d colours (label2rgb_colors)" % self.C)
        nbytes = (self.C + 1) * (self.C + 1) * 8
        self.conf_dev = self.ctx.alloc(nbytes, pooled=True)
        _lib.check(self.ctx._lib.wsc_memset(self.ctx.h, self.conf_dev.ptr, 0, nbytes))

    def close(self):
        if getattr(self, "conf_dev", None) is not None:
            self.conf_dev.free()
            self.conf_dev = None

    def _map_blocks(self, probs):
        """-> (host maps or None when they are on the device already, [(h_b, w_b)])"""
        C = self.C
        if isinstance(probs, DeviceMaps):
            if probs.dtype != np.float32 or len(probs.shape) != 4 or probs.shape[3] != C or probs.shape[0] == 0:
                raise ValueError("SegEvaluator.update: device maps %r %s must be float32 (B, h, w, %d)" % (probs.shape, probs.dtype, C))
            return None, [tuple(probs.shape[1:3])] * probs.shape[0]
        maps = [np.ascontiguousarray(p, dtype=np.float32) for p in probs]
        return maps, [tuple(m.shape[:2]) for m in maps]

    def update(self, probs, images, gts, want_pred=False, ids=None, orig_images=None):
        """probs[b] (h_b, w_b, C) float32 softmax (> 0) -- a list of host arrays, or ONE DeviceMaps (B, h, w, C) that is read in
        place (no upload); images[b] (H, W, 3) uint8 -- host arrays, or a uint8 DeviceMaps: (B, H, W, 3), or the packed ragged
        batch SegNet.preprocess_dev(keep_images=True) returns; gts[b] as seg_gt_index takes it (crf=False: or one uint8 DeviceMaps
        (B, h, w) of class indices, SegBatcher.val_batch's).
        ids (with saveimg_dir): the images' names, the debug images are written (an entry that is None is skipped: the
        reference's `j != 0` rule, :722); orig_images[b]: the decoded RGB image the reference re-reads from disk for them (:672,
        default `images`), brought to the ground truth's size; with crf=False the uint8 image to show at the map's size
        (:667 `np.uint8(img[j] + self.img_mean)`), required there.
        -> with want_pred the list of (H_b, W_b) uint8 label maps at the ground truths' sizes, else None."""
        if not self.crf:
            return self._update_argmax(probs, gts, want_pred, ids, orig_images)
        ctx, C, cfg = self.ctx, self.C, self.cfg
        dev_imgs = isinstance(images, DeviceMaps)
        B = probs.shape[0] if isinstance(probs, DeviceMaps) else len(probs)
        n_img = len(_image_blocks(images)[0]) if dev_imgs else len(images)
        if B == 0 or n_img != B or len(gts) != B:
            raise ValueError("SegEvaluator.update: %d maps, %d images, %d ground truths" % (B, n_img, len(gts)))
        maps, src_hw = self._map_blocks(probs)
        if dev_imgs:
            img_hw, img_at = _image_blocks(images)
            imgs = None
        else:
            imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
            img_hw = [tuple(im.shape[:2]) for im in imgs]
        gt = [np.ascontiguousarray(seg_gt_index(g, C, self.colours)) for g in gts]
        for b in range(B):
            if (maps is not None and (maps[b].ndim != 3 or maps[b].shape[2] != C)) or \
                    (imgs is not None and (imgs[b].ndim != 3 or imgs[b].shape[2] != 3)):
                raise ValueError("SegEvaluator.update: image %d: map %r must be (h, w, %d), image %r (H, W, 3)"
                                 % (b, maps[b].shape if maps is not None else src_hw[b], C,
                                    imgs[b].shape if imgs is not None else img_hw[b]))
            if self.resize_after_crf and img_hw[b] != src_hw[b]:
                raise ValueError("SegEvaluator.update: image %d: with resize_after_crf the image %r has the map's size %r"
                                 % (b, img_hw[b], src_hw[b]))
        out_hw = [g.shape for g in gt]
        crf_hw = src_hw if self.resize_after_crf else out_hw  # where the CRF runs
        n_out = [h * w for h, w in out_hw]
        n_crf = [h * w for h, w in crf_hw]
        prob_off = np.concatenate(([0], np.cumsum([h * w * C for h, w in src_hw])))
        crf_off = np.concatenate(([0], np.cumsum(n_crf)))  # pixels; times C: the unaries / marginals
        out_off = np.concatenate(([0], np.cumsum(n_out)))
        # one uint8 upload: [images that already have the CRF's size | images to resize | ground truths] (device images stay
        # where they are); an image that is resized lands in `res_dev`, the images of one target size next to each other (one
        # wsc_resize_u8 per size)
        todo = {}
        for b in range(B):
            if img_hw[b] != tuple(crf_hw[b]):  # (cv2.resize returns a copy otherwise)
                todo.setdefault(tuple(crf_hw[b]), []).append(b)
        rgb_at, res_at, src_at, parts, pos, res_bytes = [None] * B, [None] * B, [None] * B, [], 0, 0
        for b in range(B):
            if img_hw[b] == tuple(crf_hw[b]):
                if dev_imgs:
                    rgb_at[b] = img_at[b]
                else:
                    rgb_at[b] = pos
                    parts.append(imgs[b].reshape(-1))
                    pos += imgs[b].size
        for hw, bs in todo.items():
            for b in bs:
                res_at[b] = res_bytes
                if dev_imgs:
                    src_at[b] = img_at[b]
                else:
                    src_at[b] = pos
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
            img_ptr = images.ptr if dev_imgs else u8_dev.ptr
            prob_ptr = probs.ptr if maps is None else dev(ctx.to_device(np.concatenate([m.reshape(-1) for m in maps]), pooled=True)).ptr
            rgb_ptr = [None if rgb_at[b] is None else img_ptr + rgb_at[b] for b in range(B)]
            if todo:
                res_dev = dev(ctx.alloc(res_bytes, pooled=True))
                for hw, bs in todo.items():
                    _lib.resize_u8(ctx, img_ptr, [img_hw[b] for b in bs], [src_at[b] for b in bs], hw,
                                   res_dev.ptr + res_at[bs[0]])
                    for b in bs:
                        rgb_ptr[b] = res_dev.ptr + res_at[b]
            u_dev = dev(ctx.alloc(int(crf_off[-1]) * C * 4, pooled=True))
            _lib.seg_unary_nhwc(ctx, prob_ptr, C, src_hw, crf_hw, prob_off[:-1], crf_off[:-1] * C, u_dev)
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
            res = self._count(lab_dev, out_hw, out_off, u8_dev.ptr + gt_at, want_pred, dev)
            if self.saveimg_dir is not None and ids is not None:
                if orig_images is None:
                    orig_images = imgs if imgs is not None else [ctx.to_host(img_ptr + img_at[b], img_hw[b] + (3,), np.uint8) for b in range(B)]
                self._save_images(lab_dev, out_hw, out_off, orig_images, ids)
            return res
        finally:
            if crf is not None:
                crf.close()
            for d in bufs:
                d.free()

    def _save_images(self, lab_dev, out_hw, out_off, orig_images, ids):
        """single_crf_metrics (model.py:596-612) for a batch whose int32 label maps lie at the ground truths' sizes on the device"""
        import os

        from . import render

        ctx = self.ctx
        keep = [b for b, id_ in enumerate(ids) if id_ is not None]
        if not keep:
            return
        ids, orig_images = [ids[b] for b in keep], [orig_images[b] for b in keep]
        out_hw, lab_off = [tuple(int(v) for v in out_hw[b]) for b in keep], [int(out_off[b]) for b in keep]
        shown = render.resize_u8_grouped(ctx, orig_images, out_hw)  # :687 / :696 (a copy at equal sizes)
        show_hw = out_hw
        if self.quarter_size:
            show_hw = [render.quarter_size(hw) for hw in out_hw]
            shown = render.resize_u8_grouped(ctx, shown, show_hw)
        cols, overs = render.render_labels(ctx, lab_dev, out_hw, show_hw, self.palette, (255, 255, 255), overlay_r=0.75, label_dtype=np.int32,
                                           images=shown if self.should_overlay else None, labels_off=lab_off)
        os.makedirs(self.saveimg_dir, exist_ok=True)
        for b, id_ in enumerate(ids):
            id_ = id_.decode() if isinstance(id_, bytes) else str(id_)
            render.save_png(os.path.join(self.saveimg_dir, "%s_img.png" % id_), shown[b])
            render.save_png(os.path.join(self.saveimg_dir, "%s_output.png" % id_), overs[b] if self.should_overlay else cols[b])
            render.save_png(os.path.join(self.saveimg_dir, "%s_pred.png" % id_), cols[b])

    def _count(self, lab_dev, out_hw, out_off, gt_ptr, want_pred, dev):
        """int32 labels at the ground truths' sizes -> the confusion matrix (accumulated) and, with want_pred, the uint8 maps"""
        ctx = self.ctx
        pred_dev = dev(ctx.alloc(int(out_off[-1]), pooled=True)) if want_pred else None
        # ignore_label -1: no uint8 ground-truth index equals it, every pixel is counted
        _lib.label_confusion_nn(ctx, lab_dev, out_hw, out_hw, out_off[:-1], gt_ptr, self.C + 1, self.conf_dev,
                                pred_dev=pred_dev, ignore_label=-1)
        if want_pred:
            flat = ctx.to_host(pred_dev, (int(out_off[-1]),), np.uint8)
            return [flat[out_off[b]:out_off[b + 1]].reshape(out_hw[b]) for b in range(len(out_hw))]
        return None

    def _update_argmax(self, probs, gts, want_pred, ids=None, orig_images=None):
        """crf=False: np.argmax(pred_curr, axis=-1) of the map as it is (first maximum: wsc_seg_resize_argmax at equal sizes, on
        the class-major planes wsc_seg_planes_from_nhwc writes) and the same counting.  gts may also be ONE uint8 DeviceMaps
        (B, h, w) of class indices in [0, num_classes] (SegBatcher.val_batch): it is counted against where it lies, no host copy
        and no upload."""
        ctx, C = self.ctx, self.C
        B = probs.shape[0] if isinstance(probs, DeviceMaps) else len(probs)
        gt_on_dev = isinstance(gts, DeviceMaps)
        n_gt = gts.shape[0] if gt_on_dev else len(gts)
        if B == 0 or n_gt != B:
            raise ValueError("SegEvaluator.update: %d maps, %d ground truths" % (B, n_gt))
        maps, src_hw = self._map_blocks(probs)
        if gt_on_dev:
            if gts.dtype != np.uint8 or len(gts.shape) != 3:
                raise ValueError("SegEvaluator.update: device ground truth %r %s must be uint8 (B, h, w) class indices" % (gts.shape, gts.dtype))
            gt, gt_hw = None, [tuple(gts.shape[1:])] * B
        else:
            gt = [np.ascontiguousarray(seg_gt_index(g, C, self.colours)) for g in gts]
            gt_hw = [tuple(g.shape) for g in gt]
        for b in range(B):
            if maps is not None and (maps[b].ndim != 3 or maps[b].shape[2] != C):
                raise ValueError("SegEvaluator.update: image %d: map %r must be (h, w, %d)" % (b, maps[b].shape, C))
            if gt_hw[b] != src_hw[b]:
                raise ValueError("SegEvaluator.update: image %d: without the CRF the ground truth %r has the map's size %r"
                                 % (b, gt_hw[b], src_hw[b]))
        n_pix = [h * w for h, w in src_hw]
        out_off = np.concatenate(([0], np.cumsum(n_pix)))
        bufs = []

        def dev(buf):
            bufs.append(buf)
            return buf

        try:
            gt_ptr = gts.ptr if gt_on_dev else dev(ctx.to_device(np.concatenate([g.reshape(-1) for g in gt]), pooled=True)).ptr
            prob_ptr = probs.ptr if maps is None else dev(ctx.to_device(np.concatenate([m.reshape(-1) for m in maps]), pooled=True)).ptr
            planes = dev(ctx.alloc(int(out_off[-1]) * C * 4, pooled=True))
            if maps is None:
                _lib.seg_planes_from_nhwc(ctx, prob_ptr, B, C, n_pix[0], planes)
            else:
                for b in range(B):
                    o = int(out_off[b]) * C * 4
                    _lib.seg_planes_from_nhwc(ctx, prob_ptr + o, 1, C, n_pix[b], planes.ptr + o)
            lab_dev = dev(ctx.alloc(int(out_off[-1]) * 4, pooled=True))
            _lib.seg_resize_argmax(ctx, planes, C, src_hw, src_hw, out_off[:-1] * C, out_off[:-1], lab_dev)
            res = self._count(lab_dev, src_hw, out_off, gt_ptr, want_pred, dev)
            if self.saveimg_dir is not None and ids is not None:
                if orig_images is None or len(orig_images) != B or len(ids) != B:
                    raise ValueError("SegEvaluator.update: without the CRF the debug images need %d ids and orig_images" % B)
                self._save_images(lab_dev, src_hw, out_off, orig_images, ids)
            return res
        finally:
            for d in bufs:
                d.free()

    def metrics(self):
        conf = self.ctx.to_host(self.conf_dev, (self.C + 1, self.C + 1), np.int64)
        return seg_metrics_from_confusion(conf)


# ---- the network: create_network up to its CRF layer, and pred() (SEC.py:117-128, DSRG.py:169-186,439-452) --------------------------
SEG_TRUNK = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
             "conv5_1", "conv5_2", "conv5_3")


def seg_layer_names(method):
    """The reference's layer names of a method's network, in execution order."""
    if method == "SEC":
        return SEG_TRUNK + ("fc6", "fc7", "fc8")
    if method == "DSRG":
        return SEG_TRUNK + tuple("fc%d_%d" % (l, k) for k in (1, 2, 3, 4) for l in (6, 7, 8))
    raise ValueError("SegNet: method %r is neither 'SEC' nor 'DSRG'" % (method,))


def seg_state_dict(method, weights, num_classes):
    """{'<layer>.w': HWIO float32, '<layer>.b': float32} for wsc_net_create from either form the reference keeps weights in:
    the init-model dict {layer: {'w': HWIO, 'b': ...}} of np.load(init_model_path, allow_pickle=True).item() (SEC.py:289,
    DSRG.py:377), or a flat dict of checkpoint variables '<layer>_weights' / '<layer>_bias' (get_weights_and_bias).  A pickled
    init model has no fc8 -- the reference draws it at random -- so a missing layer raises KeyError naming it."""
    out = {}
    for layer in seg_layer_names(method):
        if layer in weights and isinstance(weights[layer], dict):
            ent = weights[layer]
            if "w" not in ent or "b" not in ent:
                raise KeyError("SegNet: weights[%r] needs 'w' and 'b'" % layer)
            w, b = ent["w"], ent["b"]
        elif layer + "_weights" in weights and layer + "_bias" in weights:
            w, b = weights[layer + "_weights"], weights[layer + "_bias"]
        else:
            raise KeyError("SegNet: no weights for layer %r (neither weights[%r]['w' / 'b'] nor '%s_weights' / '%s_bias'); an init "
                           "model has no fc8: give it explicitly" % (layer, layer, layer, layer))
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if w.ndim != 4 or w.shape[0] != w.shape[1] or b.shape[0] != w.shape[3]:
            raise ValueError("SegNet: layer %r: weights %r must be HWIO with a bias of Cout entries, got bias %r"
                             % (layer, w.shape, b.shape))
        if layer.startswith("fc8") and w.shape[3] != num_classes:
            raise ValueError("SegNet: layer %r has %d outputs, num_classes = %d" % (layer, w.shape[3], num_classes))
        out[layer + ".w"], out[layer + ".b"] = w, b
    return out


class SegNet:
    """The SEC / DSRG segmentation network on the device at drop_prob = 0: the forward pass, and the backward pass from
    d loss / d fc8 to the weight and bias gradients (forward_dev(keep=True), backward_dev, grad_step_dev).

    method 'SEC' (one fc6 / fc7 / fc8 branch at rate 12) or 'DSRG' (four ASPP branches at 6 / 12 / 18 / 24, fc8 their sum);
    weights as seg_state_dict takes them; precision _lib.PREC_F16X3 by default -- a forward whose activations leave half's range
    raises WscError(WSC_ERR_RANGE) once (the context's flag is cleared with the report): construct with _lib.PREC_F32 then."""

    def __init__(self, method, weights, num_classes, precision=_lib.PREC_F16X3, ctx=None, min_prob=1e-4):
        self.method = method
        self.C = int(num_classes)
        self.min_prob = float(min_prob)
        sd = seg_state_dict(method, weights, self.C)
        self.ctx = ctx or default_context()
        self.net = _lib.Net(self.ctx, _lib.ARCH_DEEPLAB_LFOV if method == "SEC" else _lib.ARCH_DEEPLAB_ASPP, sd, self.C, precision)
        self._sd = sd        # what the backward pass packs its data-gradient kernels from, on its first call
        self._grad = None    # _lib.SegGrad, created lazily

    def close(self):
        """Releases the packed weights.  Never raises for a pending range error: the stream is drained through the non-raising
        wsc_ctx_range_status, not wsc_sync."""
        net = getattr(self, "net", None)
        if getattr(self, "_grad", None) is not None:
            self._grad.close()
            self._grad = None
        if net is not None and getattr(net, "h", None) and self.ctx.h:
            self.ctx.range_status(clear=False)
            self.ctx._lib.wsc_net_destroy(net.h)
            net.h = None
        self.net = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def map_size(self, H, W):
        """The fc8 map size for an H x W input: (41, 41) at 321 x 321."""
        return self.net.seg_size_hw(H, W)

    def forward(self, x, want_fc8=False):
        """x (B, H, W, 3) float32 BGR minus mean -> fc8-softmax (B, h, w, C) float32; with want_fc8 also the logits."""
        ctx = self.ctx
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("SegNet: input %r must be (B, H, W, 3)" % (x.shape,))
        B, H, W, _ = x.shape
        h, w = self.map_size(H, W)
        n = B * h * w * self.C
        x_dev = ctx.to_device(x, pooled=True)
        out_dev = ctx.alloc(2 * n * 4, pooled=True)
        try:
            self.net.forward_seg(x_dev, B, H, W, out_dev.ptr, out_dev.ptr + 4 * n if want_fc8 else None, self.min_prob)
            flag = ctx.range_status(clear=True)  # drains the stream; the flag is scoped to this forward
            if flag:
                raise _lib.WscError(_lib.WSC_ERR_RANGE, "SegNet: an activation reached half's ceiling (|v| >= 65504) in a layer "
                                    "with %d output channels; use precision=_lib.PREC_F32 for this model" % flag)
            both = ctx.to_host(out_dev, (2 if want_fc8 else 1, B, h, w, self.C), np.float32)
        finally:
            x_dev.free()
            out_dev.free()
        return (both[0], both[1]) if want_fc8 else both[0]

    def softmax(self, x):
        """net['fc8-softmax']: (B, H, W, 3) float32 -> (B, h, w, C), the array generate_seed_step and SegEvaluator.update take."""
        return self.forward(x)

    def resize(self, a, size):
        """tf.image.resize_bilinear(a, size) of TensorFlow 1.x (align_corners=False) on an NHWC array, on the device."""
        ctx = self.ctx
        a = np.ascontiguousarray(a, dtype=np.float32)
        B, h, w, C = a.shape
        H, W = int(size[0]), int(size[1])
        src = ctx.to_device(a, pooled=True)
        dst = ctx.alloc(B * H * W * C * 4, pooled=True)
        try:
            _lib.resize_bilinear_tf(ctx, src, B, h, w, C, H, W, dst)
            return ctx.to_host(dst, (B, H, W, C), np.float32)
        finally:
            src.free()
            dst.free()

    def output(self, x, img_mean, crf_config, seed_size=None):
        """create_network's return value (build_crf, DSRG.py:302-335 / SEC.py:252-283): the dense-CRF layer on fc8-softmax and on
        the image x + img_mean, both brought to the seed size with the TF sampler; log-probabilities (B, s, s, C).
        seed_size None: the map's own size (41 x 41 at 321 x 321, the reference's seed_size)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        prob = self.softmax(x)
        size = prob.shape[1:3] if seed_size is None else ((seed_size, seed_size) if np.isscalar(seed_size) else tuple(seed_size))
        image = self.resize(x + np.asarray(img_mean, dtype=np.float32).reshape(1, 1, 1, 3), size)
        fmap = prob if tuple(prob.shape[1:3]) == tuple(size) else self.resize(prob, size)  # (the TF resize to the same size is the identity)
        return crf_layer(fmap, image, crf_config, self.C, min_prob=self.min_prob, ctx=self.ctx)

    def rescale_output(self, x, img_mean, crf_config, size=None, seed_size=None):
        """pred()'s net['rescale_output'] (DSRG.py:439-452): output() resized to `size`, the input's (H, W) by default."""
        out = self.output(x, img_mean, crf_config, seed_size=seed_size)
        return self.resize(out, np.shape(x)[1:3] if size is None else size)

    def preprocess(self, images, img_mean, size=(321, 321)):
        """image_preprocess of the evaluation phases (model.py:331-342): every RGB image (H, W, 3) is resized to `size` with the TF
        sampler, turned to BGR and has img_mean (BGR) subtracted -> (B, size[0], size[1], 3) float32, the network's input."""
        mean = np.asarray(img_mean, dtype=np.float32).reshape(1, 1, 3)
        out = np.empty((len(images), int(size[0]), int(size[1]), 3), np.float32)
        for i, im in enumerate(images):
            im = np.asarray(im, dtype=np.float32)
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("SegNet.preprocess: image %d is %r, not (H, W, 3)" % (i, im.shape))
            out[i] = self.resize(im[None], size)[0][:, :, ::-1] - mean
        return out

    # ---- device-resident twins: the same kernels, DeviceMaps in and out, no host array in between -----------------------------
    def _on_device(self, x):
        """-> (DeviceMaps (B, H, W, 3), the upload this call made and so frees, or None)"""
        if not isinstance(x, DeviceMaps):
            x = np.ascontiguousarray(x, dtype=np.float32)
        if len(x.shape) != 4 or x.shape[3] != 3:
            raise ValueError("SegNet: input %r must be (B, H, W, 3)" % (x.shape,))
        return device_input(self.ctx, x, np.float32, "SegNet")

    def forward_dev(self, x, want_fc8=False, keep=False, dropout=None):
        """forward() with the maps left on the device: x a DeviceMaps (B, H, W, 3) (a host array is uploaded once) ->
        DeviceMaps (B, h, w, C) fc8-softmax; with want_fc8 (softmax, logits).  The range flag as in forward(): the stream is
        drained through range_status(clear=True) and a saturated forward raises WscError(WSC_ERR_RANGE) once.
        keep: the last element returned is the tape backward_dev takes -- a SegTape: a flat float32 DeviceMaps with `.entries` (the
        plan of wsc_net_seg_tape_plan), `.input_shape` (B, H, W) and `.drop_prob`; the maps have the bits of a forward without it.
        dropout: None, or (drop_prob, seed, step) -- the training forward pass (wsc_net_forward_seg_train) with the dropout sites
        behind fc6 / fc7 active: keep-masks of (seed, step, site, element index) under the project's own counter-based contract
        (not TensorFlow's stream), the tape's fc6* / fc7* entries the dropped, scaled activations.  0.5 is
        the reference's `train` phase.  Needs keep=True: the tape is what backward_dev evaluates the chain rule at."""
        ctx = self.ctx
        if dropout is not None and not keep:
            raise ValueError("SegNet.forward_dev: dropout=%r needs keep=True (the backward pass reads the dropped tape)" % (dropout,))
        xd, mine = self._on_device(x)
        outs = []
        try:
            B, H, W, _ = xd.shape
            h, w = self.map_size(H, W)
            outs = [DeviceMaps(ctx, (B, h, w, self.C), np.float32) for _ in range(2 if want_fc8 else 1)]
            if keep:
                entries, elems = self.net.seg_tape_plan(B, H, W)
                tape = SegTape(ctx, elems, entries, (B, H, W), 0.0 if dropout is None else dropout[0])
                outs.append(tape)
                if dropout is None:
                    self.net.forward_seg_tape(xd.ptr, B, H, W, tape.ptr, elems, outs[0].ptr, outs[1].ptr if want_fc8 else None, self.min_prob)
                else:
                    drop_prob, seed, step = dropout
                    self.net.forward_seg_train(xd.ptr, B, H, W, drop_prob, seed, step, tape.ptr, elems, outs[0].ptr,
                                               outs[1].ptr if want_fc8 else None, self.min_prob)
            else:
                self.net.forward_seg(xd.ptr, B, H, W, outs[0].ptr, outs[1].ptr if want_fc8 else None, self.min_prob)
            flag = ctx.range_status(clear=True)  # drains the stream; the flag is scoped to this forward
            if flag:
                raise _lib.WscError(_lib.WSC_ERR_RANGE, "SegNet: an activation reached half's ceiling (|v| >= 65504) in a layer "
                                    "with %d output channels; use precision=_lib.PREC_F32 for this model" % flag)
        except Exception:
            for o in outs:
                o.free()
            raise
        finally:
            if mine:
                xd.free()
        return tuple(outs) if len(outs) > 1 else outs[0]

    def backward_dev(self, tape, dfc8):
        """opt.compute_gradients (wsc_net_backward_seg; wsc_net_backward_seg_drop where tape.drop_prob > 0): the tape of forward_dev(keep=True) and d loss / d fc8
        (B, h, w, C) float32 -- a DeviceMaps, e.g. the gradient loss_step_dev returns, or a host array -- -> SegGrads.  The chain rule
        evaluated at the tape, in exact fp32 whatever the net's precision.  The caller frees the result."""
        ctx, g = self.ctx, self._ensure_grad()
        B, H, W = tape.input_shape
        want = (B,) + tuple(self.map_size(H, W)) + (self.C,)
        gd, mine = device_input(ctx, dfc8, np.float32, "SegNet.backward_dev")
        out = None
        try:
            if gd.shape != want:
                raise ValueError("SegNet.backward_dev: dfc8 %r must be %r, the fc8 map's shape" % (gd.shape, want))
            out = DeviceMaps(ctx, (g.grad_elems,), np.float32)
            if tape.drop_prob == 0.0:
                g.backward(B, H, W, tape.ptr, tape.shape[0], gd.ptr, out.ptr)
            else:
                g.backward_drop(B, H, W, tape.ptr, tape.shape[0], gd.ptr, out.ptr, tape.drop_prob)
            return SegGrads(out, g.layout)
        except Exception:
            if out is not None:
                out.free()
            raise
        finally:
            if mine:
                gd.free()

    def _ensure_grad(self):
        if self._grad is None:
            self._grad = _lib.SegGrad(self.net, self._sd)
        return self._grad

    def flat_params(self, weights):
        """Weights in either form seg_state_dict takes -> one float32 array in the layout of wsc_seg_grad_layout (per layer w in
        HWIO, then b): the host form of what load_params_dev takes.  The shapes must be the net's."""
        g = self._ensure_grad()
        sd = seg_state_dict(self.method, weights, self.C)
        return _lib.flatten({layer: {"w": sd[layer + ".w"], "b": sd[layer + ".b"]} for layer in g.layout}, _lib.SegGrad.fields(g.layout), g.grad_elems)

    def load_params_dev(self, flat):
        """wsc_net_seg_load_params: every packed weight of the net and every data-gradient kernel of its backward pass rewritten on
        the device from `flat`, float32 (grad_elems,) in the layout of SegGrads -- a DeviceMaps (read in place), or a host array
        (uploaded once).  Afterwards the net has the bits of a SegNet created from those weights.  The net must not be in use on
        another context's stream during the call."""
        g = self._ensure_grad()
        fd, mine = device_input(self.ctx, flat if isinstance(flat, DeviceMaps) else np.asarray(flat).reshape(-1), np.float32, "SegNet.load_params_dev")
        try:
            if fd.shape != (g.grad_elems,):
                raise ValueError("SegNet.load_params_dev: %r must be (%d,), the layout's size" % (fd.shape, g.grad_elems))
            g.load_params(fd.ptr)
        finally:
            if mine:
                fd.free()

    def softmax_dev(self, x):
        """net['fc8-softmax'] on the device: what SegEvaluator.update and crf_layer_dev take."""
        return self.forward_dev(x)

    def resize_dev(self, a, size):
        """tf.image.resize_bilinear(a, size) of a float32 NHWC DeviceMaps -> a new DeviceMaps."""
        B, h, w, C = a.shape
        out = DeviceMaps(self.ctx, (B, int(size[0]), int(size[1]), C), np.float32)
        try:
            _lib.resize_bilinear_tf(self.ctx, a.ptr, B, h, w, C, out.shape[1], out.shape[2], out.ptr)
        except Exception:
            out.free()
            raise
        return out

    def output_dev(self, x, img_mean, crf_config, seed_size=None):
        """output() on the device: fc8-softmax, then crf_layer_dev on it and on x -> DeviceMaps (B, s_h, s_w, C)."""
        xd, mine = self._on_device(x)
        prob = None
        try:
            prob = self.softmax_dev(xd)
            return crf_layer_dev(prob, xd, img_mean, crf_config, self.C, min_prob=self.min_prob, seed_size=seed_size, ctx=self.ctx)
        finally:
            if prob is not None:
                prob.free()
            if mine:
                xd.free()

    def rescale_output_dev(self, x, img_mean, crf_config, size=None, seed_size=None):
        """rescale_output() on the device: wsc_resize_bilinear_tf of output_dev's log-probabilities to `size`, the input's (H, W)
        by default -> DeviceMaps (B, H, W, C).  (The log is taken once per seed pixel, before the resize.)"""
        xd, mine = self._on_device(x)
        try:
            with self.output_dev(xd, img_mean, crf_config, seed_size=seed_size) as out:
                return self.resize_dev(out, xd.shape[1:3] if size is None else size)
        finally:
            if mine:
                xd.free()

    def loss_step_dev(self, x, cues, labels_or_tags, img_mean, crf_config_train, seed_size=None, want_grad="fc8"):
        """The non-backward half of one training step of Model.train (model.py:464-511) at drop_prob = 0, without a host copy in
        between: forward_dev -> crf_layer_dev -> (DSRG) wsc_dsrg_seed_grow on the device buffers -> SegLoss.

        x (B, H, W, 3) the network's input, cues (B, h, w, C) the 0/1 seed cues at the map's size -- DeviceMaps, or host arrays that
        are uploaded once; labels_or_tags (B, C) or (B, 1, 1, C): SEC's labels, DSRG's tags (one array in the reference, class 0 =
        background); crf_config_train as crf_layer_dev takes it; seed_size None: the map's own size, the only one at which the
        reference's losses are defined (its seed_size is the fc8 map's 41).
        -> (losses, grad, new_cues) as SegLoss returns the first two; new_cues a float32 DeviceMaps (B, h, w, C): DSRG's grown cues
        (a new buffer), for SEC the cues themselves on the device (the caller's DeviceMaps where one was given).  The caller frees
        grad and new_cues; every other buffer of the step is freed on every path."""
        return self._loss_step(x, cues, labels_or_tags, img_mean, crf_config_train, seed_size, want_grad, False)[:3]

    def grad_step_dev(self, x, cues, labels_or_tags, img_mean, crf_config_train, seed_size=None, dropout=None):
        """One training step of Model.train up to and including compute_gradients: loss_step_dev's chain on a kept forward pass,
        then backward_dev on its gradient -> (losses, grads, new_cues): at dropout=None (drop_prob = 0) loss_step_dev's losses and
        new_cues (bit for bit), grads a SegGrads.  dropout: (drop_prob, seed, step) as forward_dev takes it.  The caller frees grads
        and new_cues; every other buffer of the step -- the tape and d loss / d fc8 among them -- is freed on every path."""
        losses, grad, new_cues, tape = self._loss_step(x, cues, labels_or_tags, img_mean, crf_config_train, seed_size, "fc8", True,
                                                       dropout=dropout)
        try:
            return losses, self.backward_dev(tape, grad), new_cues
        except Exception:
            if new_cues is not cues:
                new_cues.free()
            raise
        finally:
            grad.free()
            tape.free()

    def _loss_step(self, x, cues, labels_or_tags, img_mean, crf_config_train, seed_size, want_grad, keep, dropout=None):
        """loss_step_dev's body -> (losses, grad, new_cues, tape); tape (keep) is forward_dev's, else None"""
        ctx = self.ctx
        xd, x_mine = self._on_device(x)
        own, out = [], []  # buffers of the step, freed on every path; what the caller receives, freed on a failure only
        try:
            cd = cues
            if not isinstance(cues, DeviceMaps):
                cd = DeviceMaps.from_host(ctx, cues, dtype=np.float32)
                own.append(cd)
            tape = None
            if keep:
                prob, tape = self.forward_dev(xd, keep=True, dropout=dropout)
                out.append(tape)
            else:
                prob = self.forward_dev(xd)
            own.append(prob)
            if cd.dtype != np.float32 or cd.shape != prob.shape:
                raise ValueError("SegNet.loss_step_dev: cues %r %s must be float32 %r, the fc8 map's shape" % (cd.shape, cd.dtype, prob.shape))
            crf = crf_layer_dev(prob, xd, img_mean, crf_config_train, self.C, min_prob=self.min_prob, seed_size=seed_size, ctx=ctx)
            own.append(crf)
            if self.method == "DSRG":
                new_cues = generate_seed_step_dev(labels_or_tags, cd, prob, ctx=ctx)
                out.append(new_cues)
            else:
                new_cues = cd
                if own[0] is cd:  # uploaded here: it leaves with the result
                    out.append(own.pop(0))
            loss = SegLoss(self.method, self.C, min_prob=self.min_prob, ctx=ctx)
            loss._weights = self.__dict__.setdefault("_rank_weights", {})  # SEC's tables, cached per map size on the net
            losses, grad = loss(prob, crf, new_cues, labels=labels_or_tags if self.method == "SEC" else None, want_grad=want_grad)
            return losses, grad, new_cues, tape
        except Exception:
            for d in out:
                d.free()
            raise
        finally:
            for d in own:
                d.free()
            if x_mine:
                xd.free()

    def preprocess_dev(self, images, img_mean, size=(321, 321), keep_images=False):
        """preprocess() for the whole ragged batch in one upload of the packed uint8 images and ONE wsc_seg_preprocess_u8 launch
        -> DeviceMaps (B, size[0], size[1], 3) with preprocess()'s bits; with keep_images (that, the packed images as a uint8
        DeviceMaps carrying `sizes` and `offsets`: SegEvaluator.update takes it as its `images`)."""
        ctx = self.ctx
        imgs = [np.asarray(im) for im in images]
        for i, im in enumerate(imgs):
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("SegNet.preprocess_dev: image %d is %r, not (H, W, 3)" % (i, im.shape))
            if im.dtype != np.uint8:
                raise ValueError("SegNet.preprocess_dev: image %d is %s, not uint8 (preprocess() takes other dtypes)" % (i, im.dtype))
        if not imgs:
            raise ValueError("SegNet.preprocess_dev: no images")
        sizes = [im.shape[:2] for im in imgs]
        offsets = np.concatenate(([0], np.cumsum([im.size for im in imgs])))[:-1]
        packed = DeviceMaps.from_host(ctx, np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in imgs]))
        packed.sizes, packed.offsets = sizes, [int(o) for o in offsets]
        x = None
        try:
            x = DeviceMaps(ctx, (len(imgs), int(size[0]), int(size[1]), 3), np.float32)
            _lib.seg_preprocess_u8(ctx, packed.ptr, sizes, offsets, img_mean, x.shape[1:3], x.ptr)
        except Exception:
            packed.free()
            if x is not None:
                x.free()
            raise
        if keep_images:
            return x, packed
        packed.free()
        return x


class SegTrainer(TrainerCore):
    """One SEC / DSRG training step after another: Model.optimize() and the update branch of Model.train() (model.py:379-404,
    491-504).  drop_prob = 0.0 (the default) is the reference's phase == 'debug' graph, 0.5 its 'train' phase (SEC.py:81 /
    DSRG.py:128): dropout behind fc6 / fc7 with the keep-masks of (seed, RNG step = self.calls, site, element index) under the
    project's own counter-based contract -- not TensorFlow's random stream.  Owns a SegNet (`net`), the flat float32 parameter buffer and
    the two slot buffers (momentum, gradient accumulator) -- DeviceMaps of net._grad.grad_elems floats in SegGrads' layout, never
    downloaded by a step.  The defaults are the reference's (model.py:36-40).

    step(x, cues, labels_or_tags, img_mean, crf_config_train, epoch=None) -> (losses, new_cues)
        SegNet.grad_step_dev, then wsc_seg_sgd_accumulate (accum += mult (grad + weight_decay w) / accum_num); on every
        accum_num-th call also wsc_seg_sgd_apply (mom = mom momentum + accum, param -= lr mom, accum = 0) and
        wsc_net_seg_load_params, after which the net computes with the updated weights.  losses: grad_step_dev's, plus "l2" =
        sum of sum(w^2) / 2 over the layers (at the weights the gradient was taken at) and "total" = norm + weight_decay l2
        (model.py:383-384).  new_cues as grad_step_dev returns it; the caller frees it.  epoch: sets the rate to lr_at(epoch) first.
    lr_at(epoch)    float32(base_lr * lr_decay ** (epoch // lr_step)) (model.py:493)
    params_host()   {layer: {"w": HWIO, "b": ...}}: the init-model format SegNet takes;  momentum_host() likewise
    save(path) / SegTrainer.load(path, method, num_classes, ...)   np.save / np.load(...).item() of that dict -- the .npy
                    load_init_model reads (DSRG.py:374-377) -- with the slots under "__momentum__", "__accum__" and the step count
                    (the RNG step of the next call), rate, seed and drop_prob under "__step__" (a file without the last two loads as 0)
    close()         releases everything"""
    BUFFERS = ("params", "mom", "accum")
    SLOTS = (("__momentum__", "mom"), ("__accum__", "accum"))

    def __init__(self, method, weights, num_classes, precision=_lib.PREC_F16X3, ctx=None, base_lr=1e-4, momentum=0.9, weight_decay=5e-4,
                 accum_num=1, lr_decay=0.5, lr_step=4, min_prob=1e-4, drop_prob=0.0, seed=0):
        if int(accum_num) < 1:
            raise ValueError("SegTrainer: accum_num = %r" % (accum_num,))
        if not 0.0 <= float(drop_prob) < 1.0:
            raise ValueError("SegTrainer: drop_prob = %r is not in [0, 1)" % (drop_prob,))
        self.drop_prob, self.seed = float(drop_prob), int(seed)
        self.base_lr, self.momentum, self.weight_decay = float(base_lr), float(momentum), float(weight_decay)
        self.accum_num, self.lr_decay, self.lr_step = int(accum_num), float(lr_decay), lr_step
        self.lr = np.float32(base_lr)
        self.calls = 0
        self.net = SegNet(method, weights, num_classes, precision=precision, ctx=ctx, min_prob=min_prob)
        self.ctx = self.net.ctx
        self._init_buffers(lambda: self.net.flat_params(weights))

    @property
    def layout(self):
        return self.net._grad.layout

    def _fields(self):
        return _lib.SegGrad.fields(self.layout)

    def _flat(self, tensors):
        return self.net.flat_params(tensors)

    def close(self):
        super().close()
        if getattr(self, "net", None) is not None:
            self.net.close()
            self.net = None

    def lr_at(self, epoch):
        return np.float32(self.base_lr * self.lr_decay ** (epoch // self.lr_step))

    def step(self, x, cues, labels_or_tags, img_mean, crf_config_train, epoch=None):
        if epoch is not None:
            self.lr = self.lr_at(epoch)
        g = self.net._ensure_grad()
        dropout = (self.drop_prob, self.seed, self.calls) if self.drop_prob > 0.0 else None
        losses, grads, new_cues = self.net.grad_step_dev(x, cues, labels_or_tags, img_mean, crf_config_train, dropout=dropout)
        l2 = None
        try:
            l2 = DeviceMaps(self.ctx, (1,), np.float32)
            g.sgd_accumulate(self.params.ptr, grads.maps.ptr, self.accum.ptr, self.weight_decay, self.accum_num, l2.ptr)
            self.calls += 1
            if self.calls % self.accum_num == 0:
                g.sgd_apply(self.params.ptr, self.accum.ptr, self.mom.ptr, self.lr, self.momentum, clear_accum=True)
                g.load_params(self.params.ptr)
            l2_value = float(l2.to_host()[0])
        except Exception:
            if new_cues is not cues:
                new_cues.free()
            raise
        finally:
            grads.free()
            if l2 is not None:
                l2.free()
        losses = dict(losses)
        losses["l2"] = l2_value
        losses["total"] = losses["norm"] + self.weight_decay * l2_value
        return losses, new_cues

    def _params_dict(self):
        return self.params_host()

    def _step_dict(self):
        return {"calls": self.calls, "lr": float(self.lr), "seed": self.seed, "drop_prob": self.drop_prob}

    def _set_step(self, step):
        if step:
            self.calls, self.lr = int(step["calls"]), np.float32(step["lr"])

    @classmethod
    def load(cls, path, method, num_classes, **kwargs):
        weights, marked = cls._read(path)
        step = marked.get("__step__", {})
        # (the RNG's seed and drop_prob travel with the file, 0 where it has none; an explicit keyword wins)
        kwargs.setdefault("seed", int(step.get("seed", 0)))
        kwargs.setdefault("drop_prob", float(step.get("drop_prob", 0.0)))
        return cls(method, weights, num_classes, **kwargs)._resume(marked)


class Predictor:
    """Model.predict's loop (model.py:542-586 with eval_miou :614-739) bound to one SegNet and one SegEvaluator: update() takes the
    decoded RGB uint8 images and the ground truths of a batch and runs preprocess_dev -> softmax_dev -> SegEvaluator.update.  The
    images are uploaded once, the network's input and its maps never leave the device; without want_pred nothing is downloaded.
    The evaluator takes fc8-softmax.

    resize_after_crf=False (VOC, ADP): the CRF runs at the ground truth's size on the image as decoded (:686-689).
    resize_after_crf=True (DeepGlobe): the CRF image is `np.uint8(img[j])` of :693 -- the PREPROCESSED network input cast back to
    uint8 (wsc_seg_crf_image_u8 with a zero mean), brought to the map's size with the TF sampler since the evaluator runs that CRF
    at the map's size.  This follows the reference literally: the values are BGR minus the mean, negative ones wrap modulo 256.
    precision, ctx, weights: as SegNet takes them;  crf_config_test, colours: as SegEvaluator."""

    def __init__(self, method, weights, num_classes, crf_config_test, img_mean, size=(321, 321), colours=None, resize_after_crf=False,
                 precision=_lib.PREC_F16X3, ctx=None, saveimg_dir=None, should_overlay=True, palette=None):
        self.ctx = ctx or default_context()
        self.size = (int(size[0]), int(size[1]))
        self.img_mean = np.asarray(img_mean, dtype=np.float32).reshape(3)
        self.resize_after_crf = bool(resize_after_crf)
        self.net = self.ev = None
        self.net = SegNet(method, weights, num_classes, precision=precision, ctx=self.ctx)
        try:
            # Model.predict (:577-582): saveimg_dir = <out_dir>/predict_<category>/<layer>, should_overlay=True; DeepGlobe is the
            # dataset that runs the CRF before the resize and shows its images at a quarter (:597-600)
            self.ev = SegEvaluator(num_classes, crf_config_test, colours=colours, resize_after_crf=resize_after_crf, ctx=self.ctx,
                                   saveimg_dir=saveimg_dir, should_overlay=should_overlay, quarter_size=resize_after_crf, palette=palette)
        except Exception:
            self.close()
            raise

    def update(self, img_list, gt_list, want_pred=False, ids=None):
        """img_list[b] (H_b, W_b, 3) uint8 RGB, gt_list[b] as seg_gt_index takes it -> SegEvaluator.update's return value.
        ids: the images' names; with the constructor's saveimg_dir the three debug images per id are written."""
        ctx, held = self.ctx, []
        try:
            x, images = self.net.preprocess_dev(img_list, self.img_mean, self.size, keep_images=True)
            held += [x, images]
            prob = self.net.softmax_dev(x)
            held.append(prob)
            if self.resize_after_crf:
                B, h, w, _ = prob.shape
                images.free()
                images = DeviceMaps(ctx, (B, h, w, 3), np.uint8)
                held.append(images)
                _lib.seg_crf_image_u8(ctx, x.ptr, B, self.size[0], self.size[1], np.zeros(3, np.float32), (h, w), images.ptr)
            return self.ev.update(prob, images, gt_list, want_pred=want_pred, ids=ids, orig_images=img_list if ids is not None else None)
        finally:
            for d in held:
                d.free()

    def metrics(self):
        return self.ev.metrics()

    def close(self):
        if self.ev is not None:
            self.ev.close()
            self.ev = None
        if self.net is not None:
            self.net.close()
            self.net = None


# ---- Model.train: the batches, the shuffle order and the loop (model.py:207-348, 435-540) --------------------------------------
CRF_CONFIG_TRAIN = {"g_sxy": 3 / 12, "g_compat": 3, "bi_sxy": 80 / 12, "bi_srgb": 13, "bi_compat": 10, "iterations": 5}  # DSRG.py:77


def load_cues(path):
    """localization_cues.pickle (model.py:174-178) -> its dict: "%s_labels" % id the listed classes of an image, "%s_cues" % id
    its (3, n) index lists (class, row, col) at the seed size (:238-246)."""
    import pickle

    with open(path, "rb") as fh:
        return pickle.load(fh, encoding="iso-8859-1")


def shuffled_ids(n, seed, skip=0):
    """The order of dataset.repeat(-1).shuffle(n) (model.py:278-279) over the ids 0 .. n-1, endlessly: a buffer holds the first n
    elements of the stream 0, 1, .. n-1, 0, 1, ..; every draw picks a uniformly random slot, emits it and refills the slot with
    the stream's next element.  The draws are `np.random.default_rng(seed).integers(0, n)`, one call per emission: the project's
    own stream (as the dropout masks are), NOT TensorFlow's.  skip: the generator's state after `skip` emissions -- how a resumed
    run continues the order of the run it resumes."""
    n = int(n)
    if n < 1 or int(skip) < 0:
        raise ValueError("shuffled_ids: n = %r, skip = %r" % (n, skip))
    rng = np.random.default_rng(seed)
    buf, emitted = list(range(n)), 0  # (the stream's next element is emitted % n)
    while True:
        slot = int(rng.integers(0, n))
        out, buf[slot] = buf[slot], emitted % n
        emitted += 1
        if emitted > skip:
            yield out


def tf_nearest_index(n_in, n_out):
    """The source index of every destination index under TF 1.x resize_nearest_neighbor(align_corners=False), in float32 as
    TensorFlow computes it: scale = float32(in) / float32(out); src = min((int)floor(float32(dst) * scale), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), int(n_in) - 1)


def _tf_resize_bilinear_host(img, H, W):
    """tf.image.resize_bilinear (TF 1.x, align_corners=False) of one (h, w, c) array in float32, the products and sums of
    csrc/tf_resize.h each rounded on its own"""
    a = np.asarray(img, dtype=np.float32)
    h, w = a.shape[:2]

    def taps(n_in, n_out):
        f = np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))
        i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), f - i0.astype(np.float32)

    y0, y1, ty = taps(h, H)
    x0, x1, tx = taps(w, W)
    tx, ty = tx[None, :, None], ty[:, None, None]
    top = a[y0][:, x0] + (a[y0][:, x1] - a[y0][:, x0]) * tx
    bottom = a[y1][:, x0] + (a[y1][:, x1] - a[y1][:, x0]) * tx
    return top + (bottom - top) * ty


class SegBatcher:
    """The inputs of a SEC / DSRG training step and of a validation batch from decoded files (Model.next_batch, model.py:207-348).

    train_batch(ids, images, cues_data) -> (x, cues, labels), DeviceMaps: m_train / get_data (:229-252) -- x (B, H, W, 3) the
        network's input with SegNet.preprocess_dev's bits, cues float32 (B, s, s, C) dense from cues_data["%s_cues" % id],
        labels float32 (B, C) from cues_data["%s_labels" % id] with class 0 set.  One upload of the packed uint8 images, one
        wsc_seg_train_batch (the index lists travel in its staged table).
    val_batch(images, gts) -> (x, gt_index), DeviceMaps: m_val (:254-270) -- x through wsc_seg_preprocess_u8, gt_index uint8
        (B, H, W) in [0, C]: the ground truth (h, w), (h, w, 1) or (h, w, 3) uint8 resized with TF's nearest rule
        (tf_nearest_index) and passed through seg_gt_index's class test (wsc_seg_gt_index_tf): what SegEvaluator(crf=False)
        counts against.  One upload.
    train_batch_host / val_batch_host: the same arrays in numpy alone.
    images[b]: (h_b, w_b, 3) uint8 RGB as decoded.  colours: the (C, 3) table of the colour-coded datasets, or None (VOC)."""

    def __init__(self, num_classes, img_mean, size=(321, 321), seed_size=41, colours=None, ctx=None):
        self.ctx = ctx
        self.C = int(num_classes)
        self.img_mean = np.asarray(img_mean, dtype=np.float32).reshape(3)
        self.size = (int(size[0]), int(size[1]))
        self.seed_size = int(seed_size)
        self.colours = None if colours is None else np.ascontiguousarray(colours, dtype=np.uint8).reshape(-1, 3)
        if self.colours is not None and len(self.colours) != self.C:
            raise ValueError("SegBatcher: %d colours for %d classes" % (len(self.colours), self.C))

    @staticmethod
    def _lists(ids, cues_data):
        try:
            return [np.asarray(cues_data["%s_cues" % i]) for i in ids], [np.asarray(cues_data["%s_labels" % i]).reshape(-1) for i in ids]
        except KeyError as e:
            raise KeyError("SegBatcher: the cue file has no entry %s" % e)

    @staticmethod
    def _blocks(arrays, what, channels=(3,)):
        """uint8 arrays -> (flat views, [(h, w)], channel count)"""
        out = []
        for b, a in enumerate(arrays):
            a = np.asarray(a)
            if a.ndim == 2 and 1 in channels:
                a = a[:, :, None]
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in channels or 0 in a.shape:
                raise ValueError("SegBatcher: %s %d is %r %s, not uint8 (h, w, %s)" % (what, b, a.shape, a.dtype, " or ".join(map(str, channels))))
            out.append(np.ascontiguousarray(a))
        if not out or len({a.shape[2] for a in out}) != 1:
            raise ValueError("SegBatcher: %d %ss, one channel count for all" % (len(out), what))
        return [a.reshape(-1) for a in out], [a.shape[:2] for a in out], out[0].shape[2]

    def train_batch(self, ids, images, cues_data):
        ctx = self.ctx or default_context()
        cue_lists, label_lists = self._lists(ids, cues_data)
        flat, sizes, _ = self._blocks(images, "image")
        if len(flat) != len(cue_lists):
            raise ValueError("SegBatcher.train_batch: %d ids, %d images" % (len(cue_lists), len(flat)))
        tables = _lib.seg_cue_tables(cue_lists, label_lists)
        B, (H, W), s, C = len(flat), self.size, self.seed_size, self.C
        offsets = np.concatenate(([0], np.cumsum([f.size for f in flat])))[:-1]
        held = []
        try:
            held.append(DeviceMaps.from_host(ctx, np.concatenate(flat)))
            for shape in ((B, H, W, 3), (B, s, s, C), (B, C)):
                held.append(DeviceMaps(ctx, shape, np.float32))
            packed, x, cues, labels = held
            _lib.seg_train_batch(ctx, packed.ptr, sizes, offsets, *tables, self.img_mean, (H, W), s, C, x.ptr, cues.ptr, labels.ptr)
            held = [packed]
            return x, cues, labels
        finally:
            for d in held:
                d.free()

    def val_batch(self, images, gts):
        ctx = self.ctx or default_context()
        flat, sizes, _ = self._blocks(images, "image")
        gflat, gsizes, channels = self._blocks(gts, "ground truth", (1, 3))
        if len(flat) != len(gflat):
            raise ValueError("SegBatcher.val_batch: %d images, %d ground truths" % (len(flat), len(gflat)))
        B, (H, W) = len(flat), self.size
        offsets = np.concatenate(([0], np.cumsum([f.size for f in flat + gflat])))[:-1]
        held = []
        try:
            packed = DeviceMaps.from_host(ctx, np.concatenate(flat + gflat))
            held.append(packed)
            x = DeviceMaps(ctx, (B, H, W, 3), np.float32)
            held.append(x)
            gt = DeviceMaps(ctx, (B, H, W), np.uint8)
            held.append(gt)
            _lib.seg_preprocess_u8(ctx, packed.ptr, sizes, offsets[:B], self.img_mean, (H, W), x.ptr)
            _lib.seg_gt_index_tf(ctx, packed.ptr, gsizes, offsets[B:], channels, self.colours, self.C, (H, W), gt.ptr)
            held = [packed]
            return x, gt
        finally:
            for d in held:
                d.free()

    def _x_host(self, images):
        H, W = self.size
        mean = self.img_mean.reshape(1, 1, 3)
        return np.stack([_tf_resize_bilinear_host(im, H, W)[:, :, ::-1] - mean for im in images]).astype(np.float32)

    def train_batch_host(self, ids, images, cues_data):
        cue_lists, label_lists = self._lists(ids, cues_data)
        s, C = self.seed_size, self.C
        cues = np.zeros((len(cue_lists), s, s, C), np.float32)
        labels = np.zeros((len(cue_lists), C), np.float32)
        for b, (c, l) in enumerate(zip(cue_lists, label_lists)):
            c = c.reshape(3, -1).astype(np.int64)
            if c.size and (c.min() < 0 or c[0].max() >= C or c[1:].max() >= s):
                raise ValueError("SegBatcher: sample %d: a cue entry outside the (%d, %d, %d) plane" % (b, s, s, C))
            cues[b, c[1], c[2], c[0]] = 1.0
            labels[b, l.astype(np.int64)] = 1.0
            labels[b, 0] = 1.0
        return self._x_host(images), cues, labels

    def val_batch_host(self, images, gts):
        H, W = self.size
        out = np.empty((len(gts), H, W), np.uint8)
        for b, g in enumerate(gts):
            g = np.asarray(g)
            r = g[tf_nearest_index(g.shape[0], H)][:, tf_nearest_index(g.shape[1], W)]
            out[b] = seg_gt_index(r, self.C, None if self.colours is None else [tuple(c) for c in self.colours])
        return self._x_host(images), out


def latest_checkpoint(save_dir):
    """-> (path, i) of the epoch-<i>.npy with the largest i in save_dir (get_latest_checkpoint, model.py:406-415), or (None, 0)"""
    import os

    done = [int(f[len("epoch-"):-len(".npy")]) for f in os.listdir(save_dir)
            if f.startswith("epoch-") and f.endswith(".npy") and f[len("epoch-"):-len(".npy")].isdigit()]
    return (os.path.join(save_dir, "epoch-%d.npy" % max(done)), max(done)) if done else (None, 0)


class SegTrainLoop:
    """Model.train() (model.py:435-540): image files and the cue pickle in, checkpoints and the list of reports out.

    method, weights, num_classes: as SegTrainer takes them; weights may also be the path of an init-model .npy, or of a checkpoint
    directory (its final-0.npy, else its latest epoch-<i>.npy; the weights alone are taken from it).
    train_ids, load_image: the training images' ids and id -> decoded uint8 RGB (h, w, 3); cues_data: load_cues' dict.
    val_sets: {category: (ids, load_image, load_gt)} or None; load_gt(id) -> uint8 (h, w[, 1 | 3]).
    batch_size, max_epochs, accum_num, base_lr, lr_decay, lr_step, momentum, weight_decay: model.py:29-145 (batch size 16 is
    demo.py's default); drop_prob 0.5 is the 'train' phase; seed seeds the dropout masks and the shuffle; img_mean (BGR) is the
    dataset's; crf_config_train DSRG.py:77 / SEC.py:19; size, seed_size: the network's input and its fc8 map (321 -> 41).
    save_dir: where the checkpoints go (None: none are written); report_every: the reference's 200.

    run() -> the list of reports, {"iteration", "epoch", "lr", "seed", "constrain", "total", "miou": {category: mIoU}}.
    Per iteration i: epoch = i / iterations_per_epoch (len(train_ids) // batch_size; 0 is a ValueError), the rate is set to
    lr_at(epoch) when i % iterations_per_epoch == 0 (:493-495), then ONE SegTrainer.step on a SegBatcher.train_batch of the next
    batch_size ids of shuffled_ids(len(train_ids), seed).  Every report_every iterations, i = 0 included, a report holds the
    means of the seed / constrain / total losses since the last one (:505-511) and, per validation category, the mIoU of the
    is_eval=False pass (:520-527, :665-669, :698-719): val_batch -> SegNet.rescale_output_dev on the trainer's own net (no
    dropout) -> SegEvaluator(crf=False), once over the category's images, nothing on the host.  At every epoch boundary
    SegTrainer.save writes save_dir/epoch-<i>.npy, at the end final-0.npy (:536-538).  On start the latest epoch-<i>.npy of
    save_dir, if any, is loaded with SegTrainer.load and the loop continues at i.  Decoding runs on a small thread pool, one
    batch ahead.

    Deviations from the reference:
      1. it evaluates the logged losses in a second sess.run (:498), which pulls another batch from the iterator: its log
         describes a different batch from the one whose gradient it accumulated, and it consumes two batches per iteration.
         Here an iteration consumes one batch and the reported losses are those of the batch the gradient was taken on.
      2. its checkpoints hold the trainable variables only: on resume momentum restarts at zero and the shuffle restarts.  Here
         momentum, accumulator, RNG step and shuffle position (i * batch_size emissions) are restored: a resumed run equals the
         uninterrupted one bit for bit.  (final-0.npy is an output only; the reference would resume from it at i = 0.)
      3. the TensorBoard summaries and TF checkpoint files are out of scope.  (The debug images are written: should_saveimg with
         out_dir puts the validation's under <out_dir>/train/<i>/, see validate(); Model.predict's come from Predictor.)"""

    def __init__(self, method, weights, num_classes, train_ids, load_image, cues_data, val_sets=None, batch_size=16, max_epochs=1,
                 accum_num=1, base_lr=1e-4, lr_decay=0.5, lr_step=4, momentum=0.9, weight_decay=5e-4, drop_prob=0.5, seed=0,
                 img_mean=None, crf_config_train=None, size=(321, 321), seed_size=41, save_dir=None, report_every=200, colours=None,
                 precision=_lib.PREC_F16X3, ctx=None, num_workers=4, should_saveimg=False, out_dir=None, dataset=None, palette=None):
        import os

        self.ids, self.load_image, self.cues_data = list(train_ids), load_image, cues_data
        self.batch_size, self.max_epochs, self.report_every = int(batch_size), int(max_epochs), int(report_every)
        if self.batch_size < 1 or self.report_every < 1:
            raise ValueError("SegTrainLoop: batch_size = %r, report_every = %r" % (batch_size, report_every))
        self.per_epoch = len(self.ids) // self.batch_size
        if self.per_epoch == 0:
            raise ValueError("SegTrainLoop: %d training ids give no batch of %d" % (len(self.ids), self.batch_size))
        if img_mean is None:
            raise ValueError("SegTrainLoop: img_mean (BGR) is the dataset's and has no default")
        self.C, self.seed, self.save_dir = int(num_classes), int(seed), save_dir
        # --saveimg (model.py:513-518, :721-728): <out_dir>/train/<i>/ per report; `dataset` picks the reference's three special cases
        self.should_saveimg, self.out_dir, self.dataset = bool(should_saveimg), out_dir, str(dataset or "")
        self.palette = palette if palette is not None else colours
        self.img_mean64 = np.asarray(img_mean, dtype=np.float64).reshape(1, 1, 3)
        if self.should_saveimg and (out_dir is None or self.palette is None or len(self.palette) != int(num_classes)):
            raise ValueError("SegTrainLoop: should_saveimg needs out_dir and a palette of %d colours (label2rgb_colors)" % int(num_classes))
        self.val_sets = dict(val_sets or {})
        self.crf_cfg = dict(CRF_CONFIG_TRAIN if crf_config_train is None else crf_config_train)
        self.num_workers = max(1, int(num_workers))
        self.i, self.trainer = 0, None
        kwargs = dict(precision=precision, ctx=ctx, base_lr=base_lr, momentum=momentum, weight_decay=weight_decay, accum_num=accum_num,
                      lr_decay=lr_decay, lr_step=lr_step, drop_prob=drop_prob, seed=seed)
        resume = None
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
            resume, self.i = latest_checkpoint(save_dir)
        if resume is not None:  # (:476-484)
            self.trainer = SegTrainer.load(resume, method, num_classes, **kwargs)
        else:
            if isinstance(weights, str):  # an init-model file, or a checkpoint directory: its final-0.npy, else its latest epoch
                if os.path.isdir(weights):
                    final = os.path.join(weights, "final-0.npy")
                    weights = final if os.path.exists(final) else latest_checkpoint(weights)[0]
                    if weights is None:
                        raise ValueError("SegTrainLoop: the weights directory holds no final-0.npy and no epoch-<i>.npy")
                weights = SegTrainer._read(weights)[0]
            self.trainer = SegTrainer(method, weights, num_classes, **kwargs)
        self.batcher = SegBatcher(num_classes, img_mean, size=size, seed_size=seed_size, colours=colours, ctx=self.trainer.ctx)

    def close(self):
        if self.trainer is not None:
            self.trainer.close()
            self.trainer = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def validate(self, pool, ids, load_image, load_gt, saveimg_dir=None):
        """the mIoU of the is_eval=False pass over `ids`, in batches of batch_size (the last one may be smaller).
        saveimg_dir (the reference's --saveimg, model.py:721-728): per image `<id>_img.png`, `<id>_output.png` and `<id>_pred.png` --
        the image is `np.uint8(img[j] + self.img_mean)`, the network's own input with the mean added back (BGR; for an ADP dataset
        the channels are reversed, :724-725), the other two the label2rgb map of the arg-max (should_overlay is False in this
        call, :521-524); VOC2012 keeps the first image of every batch only (:722-723), DeepGlobe shows a quarter (:597-600)."""
        tr, bs = self.trainer, self.batch_size
        ev = SegEvaluator(self.C, None, ctx=tr.ctx, crf=False, saveimg_dir=saveimg_dir, should_overlay=False,
                          quarter_size="DeepGlobe" in self.dataset, palette=self.palette if saveimg_dir is not None else None)
        try:
            chunks = (ids[k:k + bs] for k in range(0, len(ids), bs))
            for chunk, loaded in prefetched(pool, chunks, lambda i: (load_image(i), load_gt(i))):
                x, gt = self.batcher.val_batch([d[0] for d in loaded], [d[1] for d in loaded])
                with x, gt:
                    names = shown = None
                    if saveimg_dir is not None:
                        names = [i if (j == 0 or self.dataset != "VOC2012") else None for j, i in enumerate(chunk)]
                        shown = [np.uint8(im + self.img_mean64) for im in x.to_host()]  # img_curr = np.uint8(img[j] + self.img_mean)
                        if "ADP" in self.dataset:
                            shown = [np.ascontiguousarray(im[:, :, ::-1]) for im in shown]
                    with tr.net.rescale_output_dev(x, self.batcher.img_mean, self.crf_cfg, seed_size=self.batcher.seed_size) as out:
                        ev.update(out, None, gt, ids=names, orig_images=shown)
            return ev.metrics()["mIoU"]
        finally:
            ev.close()

    def run(self):
        import os
        from concurrent.futures import ThreadPoolExecutor

        tr, bs, per_epoch = self.trainer, self.batch_size, self.per_epoch
        total = per_epoch * self.max_epochs
        order = shuffled_ids(len(self.ids), self.seed, skip=self.i * bs)
        batches = ([self.ids[next(order)] for _ in range(bs)] for _ in range(self.i, total))
        reports, sums, count = [], np.zeros(3), 0
        with ThreadPoolExecutor(max_workers=self.num_workers) as pool:
            for ids, images in prefetched(pool, batches, self.load_image):
                i = self.i
                epoch = i / per_epoch
                x, cues, labels = self.batcher.train_batch(ids, images, self.cues_data)
                with x, cues, labels:
                    losses, new_cues = tr.step(x, cues, labels, self.batcher.img_mean, self.crf_cfg,
                                               epoch=epoch if i % per_epoch == 0 else None)
                    if new_cues is not cues:
                        new_cues.free()
                sums += (losses["seed"], losses["constrain"], losses["total"])
                count += 1
                if i % self.report_every == 0:
                    means = sums / count
                    sums, count = np.zeros(3), 0
                    saveimg_dir = os.path.join(self.out_dir, "train", str(i)) if self.should_saveimg else None  # :513-518
                    miou = {cat: self.validate(pool, list(v[0]), v[1], v[2], saveimg_dir) for cat, v in self.val_sets.items()}
                    reports.append({"iteration": i, "epoch": epoch, "lr": float(tr.lr), "seed": float(means[0]),
                                    "constrain": float(means[1]), "total": float(means[2]), "miou": miou})
                    print("epoch=%f | seed_loss=%f, constrain_loss=%f, total_loss=%f" % (epoch, means[0], means[1], means[2])
                          + "".join(" | mIoU [%s] = %f" % kv for kv in miou.items()), flush=True)
                self.i = i + 1
                if self.i % per_epoch == 0 and self.save_dir is not None:
                    tr.save(os.path.join(self.save_dir, "epoch-%d.npy" % self.i))
        if self.save_dir is not None:
            tr.save(os.path.join(self.save_dir, "final-0.npy"))
        return reports


def train(*args, **kwargs):
    """SegTrainLoop(*args, **kwargs).run() with the trainer released afterwards -> the list of reports."""
    with SegTrainLoop(*args, **kwargs) as loop:
        return loop.run()
