"""01_train mirror on libwsscam: the loss head of the classifier and the score side of predict().

    ClsLoss          model.compile(loss='binary_crossentropy', metrics=['binary_accuracy', f1]) (01_train/demo.py:60-61,
                     utilities.py:69-97) on the head global pool -> Dense -> sigmoid, and the gradient of the loss through that head
                     (wsc_cls_loss; the formulas, the tie rule and the double arithmetic: include/wsscam.h)
    ScoreEvaluator   get_optimal_thresholds, get_thresholded_metrics_class, get_thresholded_metrics_overall (utilities.py:99-165)
                     on scores that stay on the device (wsc_roc_thresholds, wsc_cls_threshold_counts)
    predict          the score side of demo.py:167-205: thresholds from the validation scores, written as optimalScoreThresh into
                     <sess_id>.mat -- the file net.common.load_pretrained and keras_store.load_model read --, metrics on the split
                     `eval_on` names

    ClsTape          what a training forward pass of a plain stack keeps for its backward pass (one float32 device buffer, its plan)
    ClsGrads         the gradient of every conv / BatchNorm parameter of the stack on the device: a flat buffer, its layout,
                     name -> DeviceMaps views, to_state_dict() in torch's shapes
    grad_step        one call from a batch to every gradient of a step: net.forward_train_dev (conv -> ReLU -> BatchNorm on the batch
                     statistics, wsc_net_forward_cls_train), the loss head, net.backward_dev (wsc_net_backward_cls); with
                     dropout=(drop_prob, seed, step) the `D` sites of the stacks are active (the *_drop entry points)

    ClsTrainer       one training step after another on the device: grad_step's three passes into one resident gradient buffer, Keras'
                     SGD with Nesterov momentum (wsc_cls_sgd_step, demo.py:60) and the repack of the updated parameters into the
                     net (wsc_net_cls_load_params); drop_prob / seed: dropout at (drop_prob, seed, global_step); save / load
                     with the momentum and the dropout settings, bit-exact resume
    step_lr          the schedule of demo.py:112-113;  cyclic_lr / cyclic_session_rates: the triangular policy of demo.py:95-110
    fit              an iterable of batches through a trainer -> the per-epoch means fit_generator(verbose=2) prints

    ImageAugmenter   Keras' ImageDataGenerator as 02_cues/dataset.py:28-96 configures it: the random draws, the affine matrix, the
                     standardisation constants (the reference's 01_train/data_loader.py is missing; these are 02_cues' settings)
    ClsBatcher       flow_from_dataframe(class_mode='other'): files -> PIL decode on the host -> ONE upload of the ragged uint8
                     batch -> wsc_cls_train_batch (nearest resize, scipy's order-1 warp, flips, standardise, CHW) -> a float32
                     DeviceMaps (b, 3, H, W) and the label rows; state() / set_state() for bit-exact resume
    train            the loop of demo.py:21-127 from files to checkpoints: schedule, ClsTrainer.step per batch, validation per
                     epoch, <ckpt_dir>/<sess_id>-<epoch>.npy every lr_dropstep epochs, resume, <model_dir>/<sess_id>.npy

Dropout (the `D` entries of VGG16's layer5 and of M7's classifier branch, nn.Dropout(p=0.5)): the project's own counter-based
keep-masks, not Keras' random stream; off (drop_prob = 0.0) unless asked for.
Not here: the writing of .h5 files and TensorBoard.  Keras evaluates the loss in float32, and what it does
with the LIST class_weight of demo.py:80-82,107 is not reproduced: ClsLoss takes per-sample weights, and train passes none
(sample_weight=None)."""
import collections
import os

import numpy as np

from . import _lib
from .misc.imutils import default_context
from .device import DeviceMaps, Freed, Tape, device_operand
from .trainer import TrainerCore

K_EPSILON = 1e-7  # K.epsilon()
POOLS = {"mean": _lib.CLS_POOL_MEAN, "max": _lib.CLS_POOL_MAX}
MAX_SCORES = 16384  # wsc_roc_thresholds sorts a class in LDS

HeadGrads = collections.namedtuple("HeadGrads", "feat w bias")  # float32 DeviceMaps (B, n, F), (C, F), (C,)


def keras_metrics(values, n_elems):
    """The six values of wsc_cls_loss on B C = n_elems targets -> {'loss', 'mean_loss', 'binary_accuracy', 'f1', 'counts'}:
    binary_accuracy = K.mean(K.equal(y_true, K.round(y_pred))) and f1 formed from the counts exactly as utilities.py:69-97 writes
    it."""
    v = dict(zip(_lib.CLS_LOSS_SLOTS, (float(x) for x in values)))
    counts = {k: int(v[k]) for k in ("n_equal", "tp", "possible", "predicted")}
    recall = counts["tp"] / (counts["possible"] + K_EPSILON)
    precision = counts["tp"] / (counts["predicted"] + K_EPSILON)
    return {"loss": v["loss"], "mean_loss": v["mean_loss"], "counts": counts, "binary_accuracy": counts["n_equal"] / float(n_elems),
            "f1": 2 * ((precision * recall) / (precision + recall + K_EPSILON))}


class ClsLoss:
    """loss = ClsLoss(ctx, "mean" | "max", num_classes)          ("mean": the VGG16 head, "max": M7's)
    loss.loss_step(feat, w, bias, targets, sample_weight=None) -> {'loss', 'mean_loss', 'binary_accuracy', 'f1', 'counts'}
    loss.grad_step(...)                                        -> (that dict, HeadGrads(feat, w, bias))
      feat     (B, h, w, F) or (B, n, F): the map the head reduces (wsc_net_forward_features); w (C, F); bias (C,) or None;
               targets (B, C) 0/1 -- float32 DeviceMaps, read in place, or host arrays, uploaded once
      sample_weight  host (B,) or None (ones): 'loss' = sum_b w_b l_b / #{w_b != 0}; 'mean_loss' is the unweighted mean
      'counts' {'n_equal', 'tp', 'possible', 'predicted'}: the integers behind the two metrics
    The gradients are new float32 DeviceMaps the caller frees.  A call downloads the six loss values and nothing else."""

    def __init__(self, ctx, pool, num_classes):
        if pool not in POOLS:
            raise ValueError("ClsLoss: pool %r is neither 'mean' nor 'max'" % (pool,))
        self.ctx = ctx or default_context()
        self.pool = POOLS[pool]
        self.C = int(num_classes)
        if not 1 <= self.C <= 64:
            raise ValueError("ClsLoss: num_classes = %d (1 .. 64)" % self.C)

    def _maps(self, name, a, shape, held):
        return device_operand(self, self.ctx, name, a, np.float32, shape, held)

    def _run(self, feat, w, bias, targets, sample_weight, want_grad, out=None):
        ctx, held, grads = self.ctx, [], None
        try:
            f = self._maps("feat", feat, None, held)
            if len(f.shape) not in (3, 4) or 0 in f.shape:
                raise ValueError("ClsLoss: feat has shape %r, expected (B, h, w, F) or (B, n, F)" % (f.shape,))
            B, F = f.shape[0], f.shape[-1]
            n = int(np.prod(f.shape[1:-1]))
            wd = self._maps("w", w, (self.C, F), held)
            bd = None if bias is None else self._maps("bias", bias, (self.C,), held)
            t = self._maps("targets", targets, (B, self.C), held)
            loss_dev = DeviceMaps(ctx, (len(_lib.CLS_LOSS_SLOTS),), np.float64)
            held.append(loss_dev)
            if want_grad and out is None:
                grads = HeadGrads(DeviceMaps(ctx, f.shape), DeviceMaps(ctx, (self.C, F)), DeviceMaps(ctx, (self.C,)))
            elif want_grad:  # the caller's own buffers for w and bias (a trainer: the tail of its gradient buffer)
                gw, gb = out
                for name, g, shape in (("out[0]", gw, (self.C, F)), ("out[1]", gb, (self.C,))):
                    if not (g is None and name == "out[1]") and (not isinstance(g, DeviceMaps) or g.dtype != np.float32 or g.ctx is not ctx
                                                                  or g.ptr is None or tuple(g.shape) != shape):
                        raise ValueError("ClsLoss: %s is no live float32 DeviceMaps %r of this context" % (name, shape))
                grads = HeadGrads(DeviceMaps(ctx, f.shape), gw, gb)
            _lib.cls_loss(ctx, f.ptr, B, n, F, self.pool, wd.ptr, None if bd is None else bd.ptr, self.C, t.ptr, sample_weight,
                          loss_dev.ptr, grad_feat_dev=grads.feat.ptr if grads else None, grad_w_dev=grads.w.ptr if grads else None,
                          grad_bias_dev=grads.bias.ptr if grads and grads.bias is not None else None)
            return keras_metrics(loss_dev.to_host(), B * self.C), grads
        except Exception:
            for d in (grads or ())[:3 if out is None else 1]:  # (`out` stays the caller's)
                d.free()
            raise
        finally:
            for d in held:
                d.free()

    def loss_step(self, feat, w, bias, targets, sample_weight=None):
        return self._run(feat, w, bias, targets, sample_weight, False)[0]

    def grad_step(self, feat, w, bias, targets, sample_weight=None, out=None):
        """out: None, or (w, bias) -- float32 DeviceMaps (C, F) and (C,) (bias: or None, its gradient is then not formed) that
        receive the Linear's gradient in place of two new buffers; they stay the caller's, HeadGrads.feat is new as ever"""
        return self._run(feat, w, bias, targets, sample_weight, True, out)


class ClsTape(Tape):
    """The tape of CAM.forward_train_dev(x, keep=True): a device.Tape on the plan of Net.cls_tape_plan for a (B, 3, H, W) input;
    `dropout` None or the (drop_prob, seed, step) of the pass that wrote it (what backward_dev regenerates the keep-masks from: the
    tape itself holds no mask).  A ".stats" entry downloads as (C, 2)."""

    def __init__(self, maps, entries, B, H, W, dropout=None):
        super().__init__(maps, entries, B)
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.dropout = None if dropout is None else (float(dropout[0]), int(dropout[1]), int(dropout[2]))

    def entry_shape(self, e):
        return (e["C"] // 2, 2) if e["name"].endswith(".stats") else super().entry_shape(e)


class ClsGrads(Freed):
    """The gradient of every conv / BatchNorm parameter of a plain stack, on the device: `maps` one float32 DeviceMaps and `layout`,
    _lib.ClsGrad.layout ([{'name', 'shape', 'offset', 'size', 'conv'}] in net.common.plain_module_order; a conv weight lies as
    [3][3][Cin][Cout] at its offset).  grads[name] is a DeviceMaps view of that parameter's floats (a conv weight (3, 3, Cin, Cout),
    a vector (C,)), ptr(name) its device address; to_state_dict() downloads everything once -> {name: ndarray} in torch's shapes.
    The classifier's Linear is not here: its gradient is HeadGrads.w / .bias.  free() / a context manager releases the buffer."""

    def __init__(self, maps, layout):
        self.maps = maps
        self.layout = layout

    def _entry(self, name):
        for e in self.layout:
            if e["name"] == name:
                return e
        raise KeyError("ClsGrads: no parameter %r" % (name,))

    def keys(self):
        return [e["name"] for e in self.layout]

    def ptr(self, name):
        return self.maps.ptr + 4 * self._entry(name)["offset"]

    def __getitem__(self, name):
        e = self._entry(name)
        cout, cin = (e["shape"] + (0,))[:2]
        return self.maps.view(e["offset"], (3, 3, cin, cout) if e["conv"] else e["shape"])

    def to_state_dict(self):
        return _lib.unflatten(self.maps.to_host(), _lib.ClsGrad.fields(self.layout))


def grad_step(net, loss, x, targets, sample_weight=None, dropout=None):
    """One training step of 01_train up to the gradient of every parameter.
      net      a net.vgg16_cam.CAM / net.m7_cam.CAM with its state dict loaded; loss: a ClsLoss on the net's context whose pool is
               the net's head ("mean" VGG16, "max" M7)
      x        (B, 3, H, W) float32, a host array or a DeviceMaps of that context; targets (B, C) 0/1; sample_weight host (B,) or None
    -> (the metrics dict of ClsLoss, HeadGrads(feat, w, bias), ClsGrads): forward_train_dev on the batch statistics (the net's
    running statistics are updated with Keras' momentum 0.99), the loss head on the classifier's Linear of the state dict, and
    backward_dev.  The caller frees the two gradient objects.  The call downloads the six loss values and nothing else.
      dropout  None, or (drop_prob, seed, step): forward_train_dev's -- the dropout sites active in both passes; HeadGrads.feat
               then has the shape of the map the loss reduced (M7: the pooled, dropped layer3_p2 map)"""
    if net.ctx is not loss.ctx:
        raise ValueError("grad_step: the network lives on another context than the loss")
    w, bias = net.classifier_params(loss.C)
    feat, tape = net.forward_train_dev(x, keep=True, dropout=dropout)
    head = None
    try:
        metrics, head = loss.grad_step(feat, w, bias, targets, sample_weight)
        return metrics, head, net.backward_dev(tape, head.feat)
    except Exception:
        for m in head or ():
            m.free()
        raise
    finally:
        feat.free()
        tape.free()


def threshold_ratios(counts, n_samples):
    """int64 (C, 5) [TP, FP, TN, FN, #{target == prediction}] of n_samples samples -> {'class': {...}, 'overall': {...}} with the
    keys tpr, fpr, tnr, fnr, acc, f1: the ratios of utilities.py:132-138 per class and :157-163 over all classes.  An empty
    denominator gives nan, as numpy's division does there."""
    c = np.asarray(counts, np.int64).reshape(-1, len(_lib.CLS_COUNT_SLOTS))

    def ratios(tp, fp, tn, fn, eq, total):
        with np.errstate(divide="ignore", invalid="ignore"):
            pos, neg = tp + fn, fp + tn  # cond_positive, cond_negative
            return {"tpr": tp / pos, "fpr": fp / neg, "tnr": tn / neg, "fnr": fn / pos, "acc": eq / np.float64(total),
                    "f1": (2 * tp) / (2 * tp + fp + fn)}

    cols = [c[:, k].astype(np.float64) for k in range(c.shape[1])]
    tot = [np.float64(c[:, k].sum()) for k in range(c.shape[1])]
    return {"class": ratios(*cols, int(n_samples)), "overall": ratios(*tot, int(n_samples) * c.shape[0])}


class ScoreEvaluator:
    """The scores and targets of a prediction pass, kept on the device, and what predict() derives from them.

    ev = ScoreEvaluator(ctx, num_classes)
    ev.update(scores, targets)     scores (b, C): a float32 DeviceMaps / device buffer (the score_dev of a forward pass), copied on
                                   the device, or a host array; targets (b, C) 0/1 host array.  At most 16384 samples in all.
    ev.thresholds() -> float32 (C,)      get_optimal_thresholds: roc_curve's threshold at the first minimum of |tpr - (1 - fpr)|,
                                   +inf for a class without positives or negatives (ev.status: ROC_NO_POSITIVE / ROC_NO_NEGATIVE bits)
    ev.curves() -> [(fprs, tprs)] per class, the arrays roc_curve returns (class_fprs / class_tprs)
    ev.metrics(thresholds) -> threshold_ratios' dict, plus 'counts' int64 (C, 5)"""

    def __init__(self, ctx, num_classes):
        self.ctx = ctx or default_context()
        self.C = int(num_classes)
        if not 1 <= self.C <= 64:
            raise ValueError("ScoreEvaluator: num_classes = %d (1 .. 64)" % self.C)
        self.N = 0
        self.status = None
        self._scores = DeviceMaps(self.ctx, (MAX_SCORES, self.C))
        self._targets = DeviceMaps(self.ctx, (MAX_SCORES, self.C))

    def close(self):
        self._scores.free()
        self._targets.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def update(self, scores, targets):
        t = np.ascontiguousarray(targets, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != self.C:
            raise ValueError("ScoreEvaluator: targets have shape %r, expected (b, %d)" % (t.shape, self.C))
        b = t.shape[0]
        if self.N + b > MAX_SCORES:
            raise ValueError("ScoreEvaluator: %d + %d samples, at most %d" % (self.N, b, MAX_SCORES))
        if b == 0:
            return
        lib, ctx, at = self.ctx._lib, self.ctx, 4 * self.N * self.C
        if isinstance(scores, np.ndarray) or isinstance(scores, (list, tuple)):
            s = np.ascontiguousarray(scores, dtype=np.float32)
            if s.shape != t.shape:
                raise ValueError("ScoreEvaluator: scores have shape %r, targets %r" % (s.shape, t.shape))
            _lib.check(lib.wsc_memcpy_h2d(ctx.h, self._scores.ptr + at, s.ctypes.data, s.nbytes))
        else:
            if isinstance(scores, DeviceMaps) and (scores.dtype != np.float32 or int(np.prod(scores.shape)) != b * self.C):
                raise ValueError("ScoreEvaluator: scores are %s %r on the device, expected float32 (%d, %d)"
                                 % (scores.dtype, scores.shape, b, self.C))
            _lib.cls_scores_append(ctx, scores.ptr if isinstance(scores, DeviceMaps) else scores, b * self.C, self._scores.ptr + at)
        _lib.check(lib.wsc_memcpy_h2d(ctx.h, self._targets.ptr + at, t.ctypes.data, t.nbytes))
        ctx.sync()  # the host arrays may be temporaries
        self.N += b

    def _roc(self, curves):
        if self.N < 1:
            raise ValueError("ScoreEvaluator: no scores yet")
        ctx, C, N = self.ctx, self.C, self.N
        with DeviceMaps(ctx, (C,), np.float32) as thr, DeviceMaps(ctx, (C,), np.int32) as status, \
                DeviceMaps(ctx, (C,), np.int32) as n_points, DeviceMaps(ctx, (C, N + 1), np.int32) as fps, \
                DeviceMaps(ctx, (C, N + 1), np.int32) as tps:
            _lib.roc_thresholds(ctx, self._scores.ptr, self._targets.ptr, N, C, thr.ptr, status.ptr, n_points.ptr,
                                fps.ptr if curves else None, tps.ptr if curves else None)
            self.status = status.to_host()
            if not curves:
                return thr.to_host(), n_points.to_host(), None, None
            return thr.to_host(), n_points.to_host(), fps.to_host(), tps.to_host()

    def thresholds(self):
        return self._roc(False)[0]

    def curve_points(self):
        """-> (thresholds float32 (C,), n_points int32 (C,), fps, tps int32 (C, N + 1)): the kept points as integers"""
        return self._roc(True)

    def curves(self):
        _, n_points, fps, tps = self._roc(True)
        out = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for c in range(self.C):
                k = int(n_points[c])
                out.append((fps[c, :k] / np.float64(fps[c, k - 1]), tps[c, :k] / np.float64(tps[c, k - 1])))
        return out

    def metrics(self, thresholds):
        thr = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
        if thr.shape != (self.C,):
            raise ValueError("ScoreEvaluator: %d thresholds for %d classes" % (thr.size, self.C))
        if self.N < 1:
            raise ValueError("ScoreEvaluator: no scores yet")
        ctx = self.ctx
        with DeviceMaps.from_host(ctx, thr) as td, DeviceMaps(ctx, (self.C, len(_lib.CLS_COUNT_SLOTS)), np.int64) as cd:
            _lib.cls_threshold_counts(ctx, self._scores.ptr, self._targets.ptr, self.N, self.C, td.ptr, cd.ptr)
            counts = cd.to_host()
        out = threshold_ratios(counts, self.N)
        out["counts"] = counts
        return out


def write_thresholds(model_dir, sess_id, thresholds):
    """<model_dir>/<sess_id>.mat with optimalScoreThresh = the LIST of thresholds (demo.py:189-192: scipy.io.savemat makes it a
    (1, C) array, which net.common.load_pretrained and keras_store.load_model index) -> the path"""
    import scipy.io

    os.makedirs(model_dir, exist_ok=True)
    mat_path = os.path.join(model_dir, sess_id + ".mat")
    scipy.io.savemat(mat_path, {"optimalScoreThresh": list(thresholds)})
    return mat_path


def predict(score_batches_val, score_batches_test, model_dir, sess_id, eval_on, ctx=None):
    """The score side of predict() (01_train/demo.py:167-205).

    score_batches_val / score_batches_test: iterables of (scores, targets) batches as ScoreEvaluator.update takes them -- the scores
    of the existing forward passes (the score_dev of wsc_net_forward_cam / wsc_gap_linear_sigmoid), the targets of the split.
    The optimal thresholds of the validation scores go to <model_dir>/<sess_id>.mat as optimalScoreThresh (scipy.io.savemat of the
    list, so a (1, C) array: what load_pretrained and load_model index); the metrics are those of the split eval_on names, 'val'
    (VOC2012) or 'test' (ADP, DeepGlobe).  -> {'thresholds' float32 (C,), 'status', 'class': {...}, 'overall': {...}, 'counts',
    'curves' [(fprs, tprs)] of the evaluated split, 'mat_path'}.
    Out of scope: the .xlsx writer, the ROC plot, the X1.7 class subset and the generators."""
    if eval_on not in ("val", "test"):
        raise ValueError("predict: eval_on %r is neither 'val' nor 'test'" % (eval_on,))
    ctx = ctx or default_context()
    evs = {}
    try:
        for split, batches in (("val", score_batches_val), ("test", score_batches_test)):
            if split == "test" and eval_on != "test":
                continue
            for scores, targets in batches:
                if split not in evs:
                    evs[split] = ScoreEvaluator(ctx, np.asarray(targets).shape[1])
                evs[split].update(scores, targets)
        if "val" not in evs or eval_on not in evs:
            raise ValueError("predict: no %s batches" % ("val" if "val" not in evs else eval_on))
        thresholds = evs["val"].thresholds()
        status = evs["val"].status
        mat_path = write_thresholds(model_dir, sess_id, thresholds)
        out = evs[eval_on].metrics(thresholds)
        out.update(thresholds=thresholds, status=status, curves=evs[eval_on].curves(), mat_path=mat_path)
        return out
    finally:
        for ev in evs.values():
            ev.close()


# ---- the training loop: demo.py:60 (the optimiser), :95-113 (the schedules), fit_generator ------------------------------------------
def step_lr(epoch, latest_epoch=0, base_lr=1e-3, droprate=0.5, dropstep=20):
    """lr_scheduler of demo.py:112-113, the schedule of every call in demo.py's __main__: base_lr * droprate ** ((epoch +
    latest_epoch) // dropstep) in Python floats, rounded to the float32 Keras stores in the optimiser's `lr` variable."""
    return np.float32(base_lr * (droprate ** ((int(epoch) + int(latest_epoch)) // int(dropstep))))


def cyclic_lr(iteration, base_lr, max_lr, step_size):
    """The triangular policy of the usual clr_callback.CyclicLR (demo.py:95-110 builds it with step_size = lr_dropstep / clr_spc *
    n // batch_size): cycle = floor(1 + it / (2 step)), x = |it / step - 2 cycle + 1|, lr = base + (max - base) max(0, 1 - x), in
    float64, rounded to float32.  Batch k (counted from 0) trains at the rate of iteration k: base_lr at 0 and 2 step, max_lr at
    step.  UNPINNED: clr_callback.py is absent from the reference tree, so the iteration a batch sees (the callback sets the rate
    in on_batch_end, for the NEXT batch) cannot be held against it."""
    it, step = float(iteration), float(step_size)
    if step <= 0 or it < 0:
        raise ValueError("cyclic_lr: iteration %r, step_size %r" % (iteration, step_size))
    cycle = np.floor(1 + it / (2 * step))
    x = np.abs(it / step - 2 * cycle + 1)
    return np.float32(base_lr + (max_lr - base_lr) * np.maximum(0.0, 1 - x))


def cyclic_session_rates(session, base_lr, max_lr, droprate=0.5):
    """(base_lr, max_lr) of the 20-epoch session `session` (0, 1, ...) of demo.py:95-110: both halved (droprate) per session by
    clr._reset; cyclic_lr takes them with the iteration counted from the session's start."""
    return base_lr * droprate ** int(session), max_lr * droprate ** int(session)


class ClsTrainer(TrainerCore):
    """One 01_train step after another on the device: compile(SGD(momentum, nesterov)) + train_on_batch of demo.py:60-61.

        ClsTrainer(model, pool, num_classes, momentum=0.9, nesterov=True, bn_keep=0.99, drop_prob=0.0, seed=0)
          model      a net.vgg16_cam.CAM / net.m7_cam.CAM with its state dict loaded; the trainer trains ITS net in place
          pool       "mean" (VGG16's head) / "max" (M7's), ClsLoss's
          bn_keep    forward_train_dev's: the weight of the old running statistics (Keras' momentum 0.99)
          drop_prob, seed   > 0: step k (global_step before the step) runs forward_train_dev(dropout=(drop_prob, seed, k)) -- the
                     `D` sites of the stack under the counter-based keep-masks; the reference's models are 0.5.  0.0: no dropout,
                     the launches and bits of a trainer without the keywords
    Parameters and momentum are two resident float32 DeviceMaps of cls_grad().param_elems floats in its param_layout, initialised
    from the model's state dict and zeros; `grads` is ONE reusable gradient buffer of the same layout.  A step never downloads them.

    step(x, targets, lr, sample_weight=None) -> ClsLoss's metrics dict.  In order: forward_train_dev (the running statistics
                    move), the loss head reading the Linear from the parameter buffer's tail and writing its gradient into the
                    gradient buffer's tail, wsc_net_backward_cls into its front, wsc_cls_sgd_step at `lr`, wsc_net_cls_load_params
                    with the running statistics: afterwards the net -- training and inference form -- computes with the updated
                    parameters.  Downloads the six loss values and nothing else; frees what it allocates on every path.
                    A loss that is not finite (or a raised range flag, e.g. a NaN in x: the flag stays raised for the caller to
                    clear) is a FloatingPointError BEFORE the update is enqueued: parameters, momentum and the packed weights
                    stay as they were.  THE RUNNING STATISTICS HAVE ALREADY MOVED by then, as in any forward pass.
    global_step     steps taken (kept by save / load)
    params_host() / momentum_host()   {name: array in torch's shape}
    state_dict()    the model's full state dict with the updated tensors and running statistics; also refreshes the wrapper's own
                    copy, so the trained model and a fresh one loaded from the dict behave identically.  An M7 model's Grad-CAM
                    head is no parameter: it is the alpha the model had when the trainer was made, and travels in the dict as
                    `gradcam_weights` (drop the key to have a fresh model derive alpha from the trained weights).
    save(path) / ClsTrainer.load(path, model, pool, num_classes, ...)   np.save / np.load(...).item() of state_dict() with the
                    momentum under "__momentum__" and the step count under "__step__" -- with dropout on, `seed` and
                    `drop_prob` beside it; a resumed run continues bit for bit, dropout masks included.  load restores seed
                    and drop_prob from the file (a file without them: 0) unless the keyword is given, which wins.
                    save(path, extra={"__name__": value}) stores more keys of that form; load leaves them in `loaded_extra`
    close() / a context manager releases the three buffers (the model stays the caller's)"""
    BUFFERS = ("params", "mom", "grads")

    def __init__(self, model, pool, num_classes, momentum=0.9, nesterov=True, bn_keep=0.99, ctx=None, drop_prob=0.0, seed=0):
        self.model = model
        self.ctx = model.ctx
        if ctx is not None and ctx is not self.ctx:
            raise ValueError("ClsTrainer: the model lives on another context")
        self.loss = ClsLoss(self.ctx, pool, num_classes)
        self.momentum, self.nesterov, self.bn_keep = float(momentum), bool(nesterov), bn_keep
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError("ClsTrainer: momentum = %r (0 <= momentum < 1)" % (momentum,))
        self.drop_prob, self.seed = float(drop_prob), int(seed)
        if not 0.0 <= self.drop_prob < 1.0:  # (NaN fails both)
            raise ValueError("ClsTrainer: drop_prob = %r (0 <= drop_prob < 1)" % (drop_prob,))
        self.global_step = 0
        self.loaded_extra = {}  # (ClsTrainer.load: the file's own "__name__" keys)
        extra = model._extra_tensors(model._sd)
        if "gradcam_weights" in extra and "gradcam_weights" not in model._sd:  # M7: the head the net was built with, kept
            model._sd["gradcam_weights"] = np.ascontiguousarray(extra["gradcam_weights"], dtype=np.float32)
        self.grad = model.cls_grad()
        self._tail = {e["name"].rsplit(".", 1)[1]: e for e in self.grad.param_layout if ".classifier." in e["name"]}
        if self._tail["weight"]["shape"][0] != self.loss.C:
            raise ValueError("ClsTrainer: num_classes = %d, the net's classifier has %d rows" % (self.loss.C, self._tail["weight"]["shape"][0]))
        self._init_buffers(lambda: self.grad.flat_params(model._sd), scratch=("grads",))
        try:
            model.bn_running_dev()  # (the model's own resident buffer, made on first use: here, not inside the first step)
        except Exception:
            self.close()
            raise

    def _fields(self):
        return _lib.ClsGrad.fields(self.grad.param_layout)

    def _grad_now(self):
        return getattr(self.model, "_cls_grad", None)

    def _tail_views(self, buf):
        """(weight (C, F), bias (C,) or None): the classifier's ranges of a buffer in param_layout"""
        w, b = self._tail["weight"], self._tail.get("bias")
        return buf.view(w["offset"], w["shape"]), None if b is None else buf.view(b["offset"], b["shape"])

    def step(self, x, targets, lr, sample_weight=None):
        self._live()
        lr = float(lr)
        if not np.isfinite(lr) or lr < 0:
            raise ValueError("ClsTrainer.step: lr = %r" % (lr,))
        model, grad = self.model, self.grad
        dropout = (self.drop_prob, self.seed, self.global_step) if self.drop_prob > 0.0 else None
        feat, tape = model.forward_train_dev(x, keep=True, bn_keep=self.bn_keep, dropout=dropout)
        head = None
        try:
            w, bias = self._tail_views(self.params)
            try:
                metrics, head = self.loss.grad_step(feat, w, bias, targets, sample_weight, out=self._tail_views(self.grads))
            except _lib.WscError as e:
                if e.status != _lib.WSC_ERR_RANGE:
                    raise
                raise FloatingPointError("ClsTrainer.step: the range flag is raised (a value that is not finite, or beyond the "
                                         "precision's range, entered the net): no update") from e
            if not np.isfinite(metrics["loss"]):
                raise FloatingPointError("ClsTrainer.step: the loss is %r: no update" % (metrics["loss"],))
            if dropout is None:
                grad.backward(tape.B, tape.H, tape.W, tape.maps.ptr, tape.elems, head.feat.ptr, self.grads.ptr)
            else:
                grad.backward_drop(tape.B, tape.H, tape.W, tape.maps.ptr, tape.elems, head.feat.ptr, int(np.prod(head.feat.shape)),
                                   self.grads.ptr, *dropout)
            grad.sgd_step(self.params.ptr, self.grads.ptr, self.mom.ptr, lr, self.momentum, self.nesterov)
            model.load_params_dev(self.params)
            self.global_step += 1
            return metrics
        finally:
            for m in (feat, tape, head.feat if head else None):
                if m is not None:
                    m.free()

    def state_dict(self):
        self._live()
        sd = self.model._sd
        for k, v in self.params_host().items():
            if sd[k].shape == v.shape:
                sd[k] = v
            else:  # a Linear of more rows than the net has classes: the trained ones are the first C
                sd[k] = sd[k].copy()
                sd[k][:v.shape[0]] = v
        sd.update(self.model.bn_running())
        return {k: v.copy() for k, v in sd.items()}

    _params_dict = state_dict

    def _step_dict(self):
        step = {"global_step": self.global_step}
        if self.drop_prob > 0.0:  # (a trainer without dropout writes the file it always wrote)
            step.update(seed=self.seed, drop_prob=self.drop_prob)
        return step

    def _set_step(self, step):
        self.global_step = int(step.get("global_step", 0))

    @classmethod
    def load(cls, path, model, pool, num_classes, **kwargs):
        tensors, marked = cls._read(path)
        model.load_state_dict(tensors)
        model.cuda()
        for key, default in (("drop_prob", 0.0), ("seed", 0)):  # (the file's unless the caller says otherwise)
            kwargs.setdefault(key, marked.get("__step__", {}).get(key, default))
        return cls(model, pool, num_classes, **kwargs)._resume(marked)


def fit(trainer, batches, lr_of_step, steps_per_epoch=None):
    """`batches`: an iterable of (x, targets) or (x, targets, sample_weight), each through trainer.step at lr_of_step(k), k the
    trainer's global_step before the step (step_lr(k // steps_per_epoch, ...), cyclic_lr(k, ...)).  -> one dict per epoch of
    steps_per_epoch batches (None: the whole iterable is one epoch; a last, shorter epoch counts) with the means Keras'
    fit_generator(verbose=2) prints -- 'loss', 'binary_accuracy', 'f1', each batch weighing with its sample count (BaseLogger) --
    and 'steps', 'samples'."""
    epochs, tot, steps, seen = [], {}, 0, 0

    def flush():
        epochs.append(dict({k: v / seen for k, v in tot.items()}, steps=steps, samples=seen))

    for batch in batches:
        x, targets = batch[0], batch[1]
        m = trainer.step(x, targets, lr_of_step(trainer.global_step), batch[2] if len(batch) > 2 else None)
        n = int(x.shape[0])
        for k in ("loss", "binary_accuracy", "f1"):
            tot[k] = tot.get(k, 0.0) + m[k] * n
        steps, seen = steps + 1, seen + n
        if steps_per_epoch is not None and steps == int(steps_per_epoch):
            flush()
            tot, steps, seen = {}, 0, 0
    if steps:
        flush()
    return epochs


# ---- the generators: ImageDataGenerator + flow_from_dataframe (02_cues/dataset.py:28-96), on the device -----------------------------
class ImageAugmenter:
    """Keras' ImageDataGenerator, the part the reference configures (02_cues/dataset.py:28-96, 03c_hsn/dataset.py):

        ImageAugmenter(rotation_range=0, width_shift_range=0, height_shift_range=0, shear_range=0, zoom_range=0,
                       horizontal_flip=False, vertical_flip=False, fill_mode='nearest', cval=0.0, rescale=None, preprocessing=None)
          rotation_range, shear_range     degrees;  width / height_shift_range: a float, < 1 a fraction of the side, else pixels
                          (Keras' integer and list forms, drawn with np.random.choice, are a ValueError)
          zoom_range      z -> [1 - z, 1 + z], or (lower, upper)
          fill_mode       'nearest' / 'reflect' / 'constant' ('wrap': ValueError, wsc_cls_train_batch does not have it)
          preprocessing   None, ('sub', (r, g, b)) for x[:, :, c] -= value, or ('affine', a, b) for (x - a) / b -- the three
                          normalize() functions of dataset.py; applied BEFORE rescale, as ImageDataGenerator.standardize does
        channel_shift_range, brightness_range, the featurewise / samplewise options and zca_whitening raise ValueError: the
        reference sets none of them.

        get_random_transform(img_shape, rng) -> {'theta', 'tx', 'ty', 'shear', 'zx', 'zy', 'flip_horizontal', 'flip_vertical'}
                          from the caller's np.random.RandomState, never the global one.  Draw order: theta, tx (times the
                          height), ty (times the width), shear, (zx, zy) as ONE uniform(size=2), then the two flip coins, which
                          are drawn whether or not flipping is enabled.
        transform_matrix(params, h, w) -> float64 (3, 3) or None (identity parameters, as Keras): rotation . shift . shear . zoom
                          with numpy's dot, then transform_matrix_offset_center with o = n / 2 + 0.5.
        affine(params, h, w) -> (six doubles M00 M01 M10 M11 off0 off1 or None, flags): what wsc_cls_train_batch takes
        standardisation() -> (sub3, div, mul) float32: ((v - sub[c]) / div) * mul

    UNPINNED: the draw order and the composition are restated from the published source of keras_preprocessing 1.1
    (image/image_data_generator.py get_random_transform, image/affine_transformations.py apply_affine_transform); the package is
    not available offline, so neither can be held against it.  What IS pinned is everything after the
    matrix: PIL's resize and scipy's warp, bit for bit (tests/test_cls_batch_oracle.py).

    for_dataset('ADP' | 'VOC2012' | 'DeepGlobe', train) reproduces datagen_aug / datagen_nonaug of 02_cues/dataset.py:28-96; they
    are 02_cues' settings standing in for the reference's missing 01_train/data_loader.py."""

    def __init__(self, rotation_range=0, width_shift_range=0, height_shift_range=0, shear_range=0, zoom_range=0, horizontal_flip=False,
                 vertical_flip=False, fill_mode="nearest", cval=0.0, rescale=None, preprocessing=None, **unsupported):
        for k, v in unsupported.items():
            if k not in ("channel_shift_range", "brightness_range", "featurewise_center", "samplewise_center", "zca_whitening",
                         "featurewise_std_normalization", "samplewise_std_normalization"):
                raise TypeError("ImageAugmenter: unknown argument %r" % (k,))
            if v:
                raise ValueError("ImageAugmenter: %s is not mirrored (the reference's generators do not set it)" % k)
        for name, v in (("width_shift_range", width_shift_range), ("height_shift_range", height_shift_range)):
            if v and not isinstance(v, (float, np.floating)):
                raise ValueError("ImageAugmenter: %s = %r: only the float form is mirrored" % (name, v))
        if fill_mode not in _lib.CLS_FILL_MODES:
            raise ValueError("ImageAugmenter: fill_mode %r (one of %s)" % (fill_mode, sorted(_lib.CLS_FILL_MODES)))
        self.rotation_range, self.shear_range = rotation_range, shear_range
        self.width_shift_range, self.height_shift_range = width_shift_range, height_shift_range
        if np.isscalar(zoom_range):
            self.zoom_range = [1 - zoom_range, 1 + zoom_range]
        elif len(zoom_range) == 2:
            self.zoom_range = [zoom_range[0], zoom_range[1]]
        else:
            raise ValueError("ImageAugmenter: zoom_range %r (a float or (lower, upper))" % (zoom_range,))
        self.horizontal_flip, self.vertical_flip = bool(horizontal_flip), bool(vertical_flip)
        self.fill_mode, self.cval, self.rescale = fill_mode, float(cval), rescale
        if preprocessing is not None and not (len(preprocessing) == 2 and preprocessing[0] == "sub" and len(preprocessing[1]) == 3) \
                and not (len(preprocessing) == 3 and preprocessing[0] == "affine"):
            raise ValueError("ImageAugmenter: preprocessing %r (None, ('sub', (r, g, b)) or ('affine', a, b))" % (preprocessing,))
        self.preprocessing = preprocessing

    @classmethod
    def for_dataset(cls, dataset, train):
        if dataset == "ADP":
            return cls(horizontal_flip=train, vertical_flip=train, preprocessing=("affine", 193.09203, 56.450138 + 1e-7))
        if dataset == "VOC2012":
            aug = dict(horizontal_flip=True, width_shift_range=0.1, height_shift_range=0.1, zoom_range=0.2, rotation_range=30,
                       fill_mode="reflect") if train else {}
            return cls(rescale=1. / 255, preprocessing=("sub", (104, 117, 123)), **aug)
        if dataset.startswith("DeepGlobe"):
            return cls(rescale=1. / 255, horizontal_flip=train, vertical_flip=train)
        raise ValueError("ImageAugmenter.for_dataset: %r is none of 'ADP', 'VOC2012', 'DeepGlobe'" % (dataset,))

    def get_random_transform(self, img_shape, rng):
        if not isinstance(rng, np.random.RandomState):
            raise TypeError("ImageAugmenter.get_random_transform: rng must be the caller's np.random.RandomState")
        theta = rng.uniform(-self.rotation_range, self.rotation_range) if self.rotation_range else 0
        tx = ty = 0
        if self.height_shift_range:
            tx = rng.uniform(-self.height_shift_range, self.height_shift_range)
            if self.height_shift_range < 1:
                tx *= img_shape[0]
        if self.width_shift_range:
            ty = rng.uniform(-self.width_shift_range, self.width_shift_range)
            if self.width_shift_range < 1:
                ty *= img_shape[1]
        shear = rng.uniform(-self.shear_range, self.shear_range) if self.shear_range else 0
        if self.zoom_range[0] == 1 and self.zoom_range[1] == 1:
            zx, zy = 1, 1
        else:
            zx, zy = rng.uniform(self.zoom_range[0], self.zoom_range[1], 2)
        flip_horizontal = bool(rng.random_sample() < 0.5) and self.horizontal_flip
        flip_vertical = bool(rng.random_sample() < 0.5) and self.vertical_flip
        return {"theta": theta, "tx": tx, "ty": ty, "shear": shear, "zx": zx, "zy": zy, "flip_horizontal": flip_horizontal,
                "flip_vertical": flip_vertical}

    @staticmethod
    def transform_matrix(params, h, w):
        theta, tx, ty, shear = params.get("theta", 0), params.get("tx", 0), params.get("ty", 0), params.get("shear", 0)
        zx, zy = params.get("zx", 1), params.get("zy", 1)
        m = None
        if theta != 0:
            t = np.deg2rad(theta)
            m = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
        if tx != 0 or ty != 0:
            s = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]])
            m = s if m is None else np.dot(m, s)
        if shear != 0:
            t = np.deg2rad(shear)
            s = np.array([[1, -np.sin(t), 0], [0, np.cos(t), 0], [0, 0, 1]])
            m = s if m is None else np.dot(m, s)
        if zx != 1 or zy != 1:
            s = np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
            m = s if m is None else np.dot(m, s)
        if m is None:
            return None
        o_x, o_y = float(h) / 2 + 0.5, float(w) / 2 + 0.5
        offset = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
        reset = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
        return np.dot(np.dot(offset, m), reset)

    def affine(self, params, h, w):
        m = self.transform_matrix(params, h, w)
        flags = (_lib.CLS_FLAG_FLIP_COLS if params.get("flip_horizontal") else 0) | (_lib.CLS_FLAG_FLIP_ROWS if params.get("flip_vertical") else 0)
        if m is None:
            return None, flags
        return np.array([m[0, 0], m[0, 1], m[1, 0], m[1, 1], m[0, 2], m[1, 2]], np.float64), flags | _lib.CLS_FLAG_WARP

    def standardisation(self):
        sub, div = (0.0, 0.0, 0.0), np.float32(1.0)
        if self.preprocessing is not None and self.preprocessing[0] == "sub":
            sub = tuple(self.preprocessing[1])
        elif self.preprocessing is not None:
            sub, div = (self.preprocessing[1],) * 3, np.float32(self.preprocessing[2])
        return np.asarray(sub, np.float32), div, np.float32(1.0 if not self.rescale else self.rescale)


def _pack_images(images):
    """uint8 (H, W, 3) arrays -> (one uint8 vector, byte offsets, sizes)"""
    images = [np.asarray(a) for a in images]
    for i, a in enumerate(images):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or 0 in a.shape:
            raise ValueError("ClsBatcher: image %d is %r %s, expected uint8 (H, W, 3)" % (i, a.shape, a.dtype))
    offs = np.concatenate([[0], np.cumsum([a.size for a in images])]).astype(np.int64)
    flat = np.empty(int(offs[-1]), np.uint8)
    for a, o in zip(images, offs):
        flat[o:o + a.size] = a.reshape(-1)
    return flat, offs[:-1], [a.shape[:2] for a in images]


class ClsBatcher:
    """flow_from_dataframe(class_mode='other', target_size=(size, size)) of an ImageDataGenerator: an endless stream of batches.

        ClsBatcher(paths, labels, augmenter, size, batch_size, shuffle, seed, ctx=None)
          paths, labels   n image files and the (n, C) label array;  size: an int or (H, W)
          shuffle, seed   the order of an epoch is a permutation from the batcher's OWN np.random.RandomState(seed) (False:
                          0 .. n - 1); the same generator then draws every sample's transform, in batch order
        .n, .data (the (n, C) float32 label array demo.py:80 sums), len() = ceil(n / batch_size); the last batch of an epoch is
        the shorter one, and the next epoch begins behind it.
        next(batcher) -> (x, labels): x a float32 DeviceMaps (b, 3, H, W) the caller frees, labels the (b, C) host rows.  Decoding
        is PIL on the host (load_img: convert('RGB')); then ONE upload of the ragged uint8 batch and wsc_cls_train_batch.
        plan()          the host half of a batch -> (indices, affine (b, 6) float64, flags (b,) int32); advances the state
        apply(images, affine, flags) -> x: the device half on decoded uint8 (H, W, 3) arrays
        state() / set_state(s)   epoch, position, the epoch's order and the generator's state: a batcher set to a saved state
                          continues bit for bit
        Everything a call allocates is freed on every path, x excepted on success."""

    def __init__(self, paths, labels, augmenter, size, batch_size, shuffle, seed, ctx=None):
        self.paths = list(paths)
        self.data = np.ascontiguousarray(labels, dtype=np.float32)
        self.n = len(self.paths)
        if self.n < 1 or self.data.ndim != 2 or self.data.shape[0] != self.n:
            raise ValueError("ClsBatcher: %d paths, labels of shape %r" % (self.n, self.data.shape))
        self.augmenter = augmenter
        self.hw = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        self.batch_size = int(batch_size)
        if self.batch_size < 1 or min(self.hw) < 1:
            raise ValueError("ClsBatcher: batch_size %r, size %r" % (batch_size, size))
        self.shuffle = bool(shuffle)
        self._ctx = ctx
        self.rng = np.random.RandomState(seed)
        self.epoch, self.pos, self.order = 0, 0, None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def reset(self):
        """back to the first batch of the current order's epoch (an unshuffled pass over a validation split)"""
        self.pos = 0

    def state(self):
        return {"epoch": self.epoch, "pos": self.pos, "order": None if self.order is None else self.order.copy(),
                "rng": self.rng.get_state()}

    def set_state(self, s):
        self.epoch, self.pos = int(s["epoch"]), int(s["pos"])
        self.order = None if s["order"] is None else np.array(s["order"], np.int64)
        self.rng.set_state(s["rng"])

    def plan(self):
        if self.order is None or self.pos >= self.n:
            if self.order is not None:
                self.epoch += 1
            self.order = self.rng.permutation(self.n).astype(np.int64) if self.shuffle else np.arange(self.n, dtype=np.int64)
            self.pos = 0
        idx = self.order[self.pos:self.pos + self.batch_size]
        self.pos += len(idx)
        H, W = self.hw
        affine, flags = np.zeros((len(idx), 6), np.float64), np.zeros(len(idx), np.int32)
        for k in range(len(idx)):
            a, flags[k] = self.augmenter.affine(self.augmenter.get_random_transform((H, W, 3), self.rng), H, W)
            if a is not None:
                affine[k] = a
        return idx, affine, flags

    def decode(self, idx):
        from PIL import Image

        out = []
        for i in idx:
            with Image.open(self.paths[int(i)]) as im:
                out.append(np.asarray(im if im.mode == "RGB" else im.convert("RGB"), dtype=np.uint8))
        return out

    def apply(self, images, affine, flags):
        H, W = self.hw
        flat, offs, sizes = _pack_images(images)
        sub, div, mul = self.augmenter.standardisation()
        ctx, src, x = self.ctx, None, None
        try:
            src = DeviceMaps.from_host(ctx, flat)
            x = DeviceMaps(ctx, (len(images), 3, H, W), np.float32)
            _lib.cls_train_batch(ctx, src.ptr, sizes, offs, (H, W), affine, flags, self.augmenter.fill_mode, self.augmenter.cval, sub, div,
                                 mul, x.ptr)
            return x
        except Exception:
            if x is not None:
                x.free()
            raise
        finally:
            if src is not None:  # (pooled: reuse is ordered behind the launch on the context's stream)
                src.free()

    def __iter__(self):
        return self

    def __next__(self):
        idx, affine, flags = self.plan()
        return self.apply(self.decode(idx), affine, flags), self.data[idx]


def find_latest_checkpoint(filedir, sess_id):
    """utilities.py:60-67 for the '<sess_id>-<epoch:02d>.npy' files train writes: the newest file (two of one timestamp: the
    later epoch) -> (path, epoch), or (None, 0)"""
    found = []
    for name in os.listdir(filedir) if os.path.isdir(filedir) else []:
        stem, ext = os.path.splitext(name)
        if ext == ".npy" and "-" in stem and "-".join(stem.split("-")[:-1]) == sess_id and stem.split("-")[-1].isdigit():
            path = os.path.join(filedir, name)
            found.append((os.path.getmtime(path), int(stem.split("-")[-1]), path))
    if not found:
        return None, 0
    found.sort()
    return found[-1][2], found[-1][1]


def train_schedule(n, batch_size, should_clr=False, base_lr=1e-3, lr_dropstep=20, lr_droprate=0.5, clr_base_lr=1e-3, clr_max_lr=2e-2,
                   clr_spc=4):
    """-> rate(epoch, k): the float32 learning rate of batch k (from 0) of epoch `epoch` (from 0, counted over resumes) in train:
    step_lr(epoch) per epoch (demo.py:112-113), or with should_clr the triangular policy in sessions of lr_dropstep epochs
    (demo.py:95-110): cyclic_lr(iteration counted from the session's start, *cyclic_session_rates(session), step_size) with
    step_size = lr_dropstep / clr_spc * n // batch_size, the reference's expression."""
    steps = int(n) // int(batch_size)
    step_size = lr_dropstep / clr_spc * n // batch_size

    def rate(epoch, k):
        if not should_clr:
            return step_lr(epoch, 0, base_lr, lr_droprate, lr_dropstep)
        session, within = divmod(int(epoch), int(lr_dropstep))
        lo, hi = cyclic_session_rates(session, clr_base_lr, clr_max_lr, lr_droprate)
        return cyclic_lr(within * steps + int(k), lo, hi, step_size)

    return rate


def _validate(model, trainer, batcher):
    """One unshuffled pass of `batcher` over its split through the net's inference feature pass (wsc_net_forward_features: the
    running statistics) and ClsLoss.loss_step on the trainer's Linear -> {'val_loss', 'val_binary_accuracy', 'val_f1'}, each
    batch weighing with its sample count."""
    H, W = batcher.hw
    if H != W:
        raise ValueError("train: the inference feature pass takes square inputs, not %dx%d" % (H, W))
    net, ctx = model._ensure_net(), model.ctx
    h, F = net.cam_size(H), net.feat_channels()
    w, bias = trainer._tail_views(trainer.params)
    tot, seen = {"loss": 0.0, "binary_accuracy": 0.0, "f1": 0.0}, 0
    batcher.reset()
    for _ in range(len(batcher)):
        x, targets = next(batcher)
        try:
            b = x.shape[0]
            with DeviceMaps(ctx, (b, h, h, F), np.float32) as feat:
                net.forward_features(x.ptr, b, H, feat.ptr)
                m = trainer.loss.loss_step(feat, w, bias, targets)
        finally:
            x.free()
        for k in tot:
            tot[k] += m[k] * b
        seen += b
    return {"val_" + k: v / seen for k, v in tot.items()}


def train(paths, labels, val_paths, val_labels, model, pool, sess_id, model_dir, ckpt_dir, epochs, batch_size, should_clr=False, seed=0,
          size=321, augmenter="VOC2012", val_augmenter=None, base_lr=1e-3, lr_dropstep=20, lr_droprate=0.5, momentum=0.9,
          clr_base_lr=1e-3, clr_max_lr=2e-2, clr_spc=4, drop_prob=0.0):
    """train() of 01_train/demo.py:21-127 from image files to checkpoints, on the device.

      paths, labels / val_paths, val_labels   the image files and (n, C) 0/1 label arrays of the two splits (gen_train, gen_val)
      model, pool     a net.vgg16_cam.CAM / net.m7_cam.CAM with its state dict loaded, and its head ("mean" / "max"): ClsTrainer's
      augmenter       an ImageAugmenter or a dataset name for ImageAugmenter.for_dataset(name, train=True); val_augmenter: the
                      same for the validation split (default: the non-augmenting generator of that dataset)
      size            img_size of demo.py:29-32 (321 VGG16, 224 the M nets)
      drop_prob       ClsTrainer's, with `seed` (the batcher's seed as well) as the masks' seed: THE REFERENCE'S MODELS ARE 0.5
                      (nn.Dropout(p=0.5), common_cnn.py:133-134); the default 0.0 leaves dropout off, the launches and bits of a
                      call without the keyword (nothing is passed to the trainer: a run resumed from a checkpoint continues with
                      the checkpoint's own drop_prob and seed).  A resumed run continues with the checkpoint's step counter, so
                      its masks are those of the uninterrupted run.  Validation is the inference feature pass: never dropped.
    steps_per_epoch = n // batch_size batches of ONE endless ClsBatcher(shuffle=True, seed) per epoch, as fit_generator draws them
    (the short last batch of a pass opens the next epoch); every batch through ClsTrainer.step(x, labels, rate, None) at
    train_schedule's rate; after every epoch _validate on the WHOLE validation split in file order (the reference's
    validation_steps = n // batch_size of a never-reset iterator drifts through the split instead).  Every lr_dropstep epochs
    <ckpt_dir>/<sess_id>-<epoch:02d>.npy = ClsTrainer.save plus the epoch and the batcher's state; a run finds the latest one
    (find_latest_checkpoint) and continues from it bit for bit.  At the end <model_dir>/<sess_id>.npy is the state dict.
    -> one dict per epoch run: {'epoch' (from 1), 'lr' (the last batch's), 'loss', 'binary_accuracy', 'f1', 'val_loss',
    'val_binary_accuracy', 'val_f1', 'steps', 'samples'}.
    Not mirrored: validation_steps = n // batch_size (the whole split is validated, see above), class_weight
    (sample_weight=None), Keras' random stream behind the dropout masks, the .h5 / .hdf5 formats, the .json architecture file,
    TensorBoard."""
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    n, C = labels.shape
    epochs, batch_size, lr_dropstep = int(epochs), int(batch_size), int(lr_dropstep)
    steps = n // batch_size
    if epochs < 1 or batch_size < 1 or steps < 1:
        raise ValueError("train: epochs %d, batch_size %d, %d samples" % (epochs, batch_size, n))
    if isinstance(augmenter, str):
        if val_augmenter is None:
            val_augmenter = ImageAugmenter.for_dataset(augmenter, False)
        augmenter = ImageAugmenter.for_dataset(augmenter, True)
    if val_augmenter is None:
        raise ValueError("train: an ImageAugmenter for the training split needs a val_augmenter")
    for d in (model_dir, ckpt_dir):
        os.makedirs(d, exist_ok=True)
    drop = {"drop_prob": drop_prob, "seed": 0 if seed is None else seed} if drop_prob else {}  # (0.0: the trainer's own defaults)
    rate = train_schedule(n, batch_size, should_clr, base_lr, lr_dropstep, lr_droprate, clr_base_lr, clr_max_lr, clr_spc)
    latest, latest_epoch = find_latest_checkpoint(ckpt_dir, sess_id)
    if latest is not None:
        trainer = ClsTrainer.load(latest, model, pool, C, momentum=momentum, nesterov=True, **drop)
    else:
        model.cuda()
        trainer = ClsTrainer(model, pool, C, momentum=momentum, nesterov=True, **drop)
    history = []
    try:
        gen = ClsBatcher(paths, labels, augmenter, size, batch_size, True, seed, ctx=trainer.ctx)
        gen_val = ClsBatcher(val_paths, val_labels, val_augmenter, size, batch_size, False, seed, ctx=trainer.ctx)
        if latest is not None:
            saved = trainer.loaded_extra["__train__"]
            latest_epoch = int(saved["epoch"])
            gen.set_state(saved["batcher"])
        for epoch in range(latest_epoch, epochs):
            tot, seen, lr = {"loss": 0.0, "binary_accuracy": 0.0, "f1": 0.0}, 0, None
            for k in range(steps):
                x, targets = next(gen)
                try:
                    lr = rate(epoch, k)
                    m = trainer.step(x, targets, lr, None)
                finally:
                    x.free()
                for key in tot:
                    tot[key] += m[key] * len(targets)
                seen += len(targets)
            row = dict({key: v / seen for key, v in tot.items()}, epoch=epoch + 1, lr=float(lr), steps=steps, samples=seen)
            row.update(_validate(model, trainer, gen_val))
            history.append(row)
            if (epoch + 1) % lr_dropstep == 0:
                trainer.save(os.path.join(ckpt_dir, "%s-%02d.npy" % (sess_id, epoch + 1)),
                             extra={"__train__": {"epoch": epoch + 1, "batcher": gen.state()}})
        TrainerCore._write(os.path.join(model_dir, sess_id + ".npy"), trainer.state_dict())
        return history
    finally:
        trainer.close()
