"""03b_irn/step/train_irn.py on libwsscam: the loss of one training step and the gradient it sends into the two head outputs.

    AffinityLoss   AffinityDisplacementLoss.forward's four loss tensors (net/resnet50_irn.py:198-213), the pair labels the
                   affinity datasets attach (GetAffinityLabelFromIndices, voc12/dataloader.py:115-131) and the reductions of
                   step/train_irn.py:114-125 in one device call (wsc_irn_aff_loss; the formulas, the tie rules and the double
                   arithmetic: include/wsscam.h), with d total / d edge_out and d total / d dp_out.  loss_step chains it behind
                   EdgeDisplacement.forward_train_dev (Net.forward in training mode); grad_step adds the backward pass of the
                   heads (EdgeDisplacement.backward_dev, wsc_net_backward_edge) on a kept tape: total_loss.backward().
    EdgeTape       what a forward pass keeps for that backward pass (one float32 device buffer and its plan)
    IrnGrads       the gradient of every trainable parameter on the device: a flat buffer, its layout, to_state_dict() in
                   torch's shapes, and `groups`, the two name lists of trainable_parameters() (train_irn's lr and 10 lr groups)
    reduce_label   the IR label at the resolution of the head outputs (voc12/dataloader.py:317)

    IrnTrainer     train_irn.run's loop end to end: grad_step, the PolyOptimizer update (misc.torchutils.PolyOptimizer,
                   wsc_irn_sgd_step) and the repack of the head weights into the net (wsc_net_irn_load_params) per step, the
                   closing dp_mean pass (fit_dp_mean, train_irn.py:148-164), and the trained state dict

    TrainBatcher   what feeds a step: the affinity datasets' rescale / normalise / flip / crop and the quarter-size label
                   (voc12/dataloader.py:270-321) from decoded files, on the device (wsc_irn_train_batch); step.train_irn.run is
                   the loop around it (shuffled epochs, drop_last)

Every backbone stage is detached in Net.forward, so the gradient of the heads is the whole gradient of a step.  DataParallel is
not here."""
import numpy as np

from . import _lib
from .misc import imutils
from .misc.torchutils import PolyOptimizer
from .device import DeviceMaps, Freed, Tape, device_operand
from .trainer import TrainerCore


def reduce_label(label):
    """imutils.pil_rescale(label, 0.25, 0) (voc12/dataloader.py:317, and the ADP / DeepGlobe twins): the (H, W) uint8 IR label
    of cam_to_ir_label, nearest-neighbour, at a quarter of the crop -- the resolution of edge_out and dp_out."""
    label = np.asarray(label)
    if label.ndim != 2:
        raise ValueError("reduce_label: label has shape %r, expected (H, W)" % (label.shape,))
    return np.ascontiguousarray(imutils.pil_rescale(label.astype(np.uint8), 0.25, 0))


class EdgeTape(Tape):
    """The tape of EdgeDisplacement.forward_train_dev(x, keep=True): a device.Tape on the plan of Net.edge_tape_plan for N samples
    of S x S."""

    def __init__(self, maps, entries, N, S):
        super().__init__(maps, entries, N)
        self.N, self.S = int(N), int(S)


class IrnGrads(Freed):
    """The gradient of every trainable parameter of an EdgeDisplacement net, on the device: `maps` one float32 DeviceMaps and
    `layout`, _lib.IrnGrad.layout ([{'name', 'shape', 'offset', 'size', 'conv'}] in the order of trainable_parameters(); a conv
    weight lies as [Cin][Cout] at its offset).  ptr(name) is a parameter's device address; to_state_dict() downloads everything
    once -> {name: ndarray} in torch's shapes; groups = (edge names, dp names): train_irn.py:60-65 gives the first lr, the second
    10 lr.  free() / a context manager releases the buffer."""

    def __init__(self, maps, layout):
        self.maps = maps
        self.layout = layout
        self.groups = ([e["name"] for e in layout if e["name"].startswith("fc_edge")],
                       [e["name"] for e in layout if not e["name"].startswith("fc_edge")])

    def ptr(self, name):
        return self.maps.ptr + 4 * next(e for e in self.layout if e["name"] == name)["offset"]

    def to_state_dict(self):
        return _lib.unflatten(self.maps.to_host(), _lib.IrnGrad.fields(self.layout))


class AffinityLoss:
    """The IRNet training loss on the device.

    loss = AffinityLoss(path_index, valid_below=21, ctx=None)       path_index: misc.indexing.PathIndex (train_irn.py:16: radius 10)
    losses, grad_edge, grad_dp = loss(edge_out, dp_out, label, want_grad=True)
      edge_out  (B, h, w) or (B, 1, h, w) float32: the edge logits, BEFORE the sigmoid
      dp_out    (B, 2, h, w) float32
      label     (B, h, w) uint8: the reduced IR labels (reduce_label), 255 = ignore; labels >= valid_below are ignored too
                -- each a DeviceMaps, read in place, or a host array, uploaded once
      -> ({"pos_bg", "pos_fg", "pos", "neg", "dp_fg", "dp_bg", "total", "n_bg", "n_fg", "n_neg"} as Python floats: train_irn's
          bg_pos_aff_loss, fg_pos_aff_loss, loss1 .. loss4, total_loss and the three pair counts,
          d total / d edge_out as a new float32 DeviceMaps of edge_out's shape, d total / d dp_out likewise; None, None when
          want_grad is false)
    The call downloads the ten loss values and nothing else."""

    def __init__(self, path_index, valid_below=21, ctx=None):
        self.radius_floor = int(path_index.radius_floor)
        self.tables = path_index.device_tables()
        self.valid_below = int(valid_below)
        if not 1 <= self.valid_below <= 255:
            raise ValueError("AffinityLoss: valid_below = %d (1 .. 255; 255 is the ignore label)" % self.valid_below)
        self.ctx = ctx or imutils.default_context()

    def _maps(self, name, a, dtype, shape, held):
        return device_operand(self, self.ctx, name, a, dtype, shape, held)

    def __call__(self, edge_out, dp_out, label, want_grad=True):
        ctx, held, grads = self.ctx, [], []
        try:
            e = self._maps("edge_out", edge_out, np.float32, lambda s: (len(s) == 3 or (len(s) == 4 and s[1] == 1)) and 0 not in s, held)
            B, h, w = e.shape[0], e.shape[-2], e.shape[-1]
            d = self._maps("dp_out", dp_out, np.float32, (B, 2, h, w), held)
            lab = self._maps("label", label, np.uint8, (B, h, w), held)
            loss_dev = DeviceMaps(ctx, (len(_lib.IRN_LOSS_SLOTS),), np.float64)
            held.append(loss_dev)
            if want_grad:
                grads.append(DeviceMaps(ctx, e.shape, np.float32))
                grads.append(DeviceMaps(ctx, d.shape, np.float32))
            dirs, start, yx = self.tables
            _lib.irn_aff_loss(ctx, e.ptr, d.ptr, lab.ptr, B, h, w, dirs, start, yx, self.radius_floor, self.valid_below, loss_dev.ptr,
                              grad_edge_dev=grads[0].ptr if want_grad else None, grad_dp_dev=grads[1].ptr if want_grad else None)
            values = loss_dev.to_host()
            losses = {k: float(v) for k, v in zip(_lib.IRN_LOSS_SLOTS, values)}
            return (losses, grads[0], grads[1]) if want_grad else (losses, None, None)
        except Exception:
            for g in grads:
                g.free()
            raise
        finally:
            for m in held:
                m.free()

    def loss_step(self, net, x, label, want_grad=True, keep=False):
        """One training step up to the gradient of the head outputs: net.forward_train_dev(x) (an EdgeDisplacement wrapper; x
        (B, 3, S, S)), then this loss on its outputs -> (losses, grad_edge, grad_dp, edge_out, dp_out), the last four DeviceMaps
        the caller frees (the gradients None when want_grad is false); keep=True: the forward pass keeps its tape (the same
        launches and bits) and the EdgeTape comes sixth.  `net` must live on this loss's context."""
        if net.ctx is not self.ctx:
            raise ValueError("AffinityLoss.loss_step: the network lives on another context than the loss")
        outs = net.forward_train_dev(x, keep=True) if keep else net.forward_train_dev(x)
        edge, dp = outs[0], outs[1]
        try:
            if edge.shape[1:] != dp.shape[2:]:
                raise ValueError("AffinityLoss.loss_step: edge_out is %r and dp_out %r: the loss needs one resolution" % (edge.shape, dp.shape))
            losses, g_edge, g_dp = self(edge, dp, label, want_grad=want_grad)
        except Exception:
            for m in outs:
                m.free()
            raise
        return (losses, g_edge, g_dp) + tuple(outs)

    def grad_step(self, net, x, label):
        """One training step up to the gradient of every trainable parameter: loss_step on a kept tape, then net.backward_dev
        -> (losses, IrnGrads); the caller frees the IrnGrads.  Everything else the step allocated is freed on every path."""
        losses, g_edge, g_dp, edge, dp, tape = self.loss_step(net, x, label, keep=True)
        try:
            return losses, net.backward_dev(tape, g_edge, g_dp)
        finally:
            for m in (g_edge, g_dp, edge, dp, tape):
                m.free()


class TrainBatcher:
    """One training batch on the device from decoded files: the sample transform of the *AffinityDataset classes
    (voc12/dataloader.py:270-321 and twins) as wsc_irn_train_batch, bit for bit what the host datasets' item() returns.

        TrainBatcher(ctx, crop_size, norm_mode, outsize=None, normalize=None, rescale=None)
          norm_mode   'int' / 'float' of TorchvisionNormalize; normalize: the dataset's TorchvisionNormalize class (its
                      constants differ per dataset; default voc12.dataloader's)
          outsize     None: the records' (scaled_h, scaled_w) are the target of the PIL rescale (stage 1; a sample that has that
                      size already is left alone); (h, w): TorchvisionResize of image and label to it (stage 2: vgg16 / m7)
          rescale     the dataset's scale range, only checked: rescale together with outsize is a ValueError (no reference
                      configuration combines them)
        apply(images, labels, params) -> (x float32 (B,3,S,S), label uint8 (B,S,S), reduced uint8 (B,s,s)), three DeviceMaps
          images      B uint8 (H, W, 3) arrays, labels B uint8 (H, W) arrays (dataset.decoded), params B records (dataset.draw)
          One upload of the packed images, one of the packed labels, no download; the caller frees the three results.
          x and reduced are what IrnTrainer.step(x, reduced) takes."""

    def __init__(self, ctx, crop_size, norm_mode, outsize=None, normalize=None, rescale=None):
        if rescale and outsize is not None:
            raise ValueError("TrainBatcher: rescale together with outsize: no reference configuration combines them")
        if normalize is None:
            from .voc12.dataloader import TorchvisionNormalize as normalize
        if norm_mode not in ("int", "float"):
            raise ValueError("norm_mode value is not 'int' or 'float'")
        self.ctx = ctx
        self.crop_size = int(crop_size)
        self.reduced_size = _lib.irn_reduced_size(self.crop_size)
        self.norm = normalize(norm_mode)
        self.pre_div255 = norm_mode == "float"
        self.outsize = None if outsize is None else (int(outsize[0]), int(outsize[1]))
        self.stage = _lib.IRN_STAGE_PIL_RESCALE if self.outsize is None else _lib.IRN_STAGE_TV_RESIZE

    @staticmethod
    def _pack(name, arrays, ndim):
        """-> (one uint8 vector, byte offsets, sizes)"""
        arrays = [np.asarray(a) for a in arrays]
        for i, a in enumerate(arrays):
            if a.dtype != np.uint8 or a.ndim != ndim or (ndim == 3 and a.shape[2] != 3) or 0 in a.shape:
                raise ValueError("TrainBatcher: %s %d is %r %s, expected uint8 %s" % (name, i, a.shape, a.dtype, "(H, W, 3)" if ndim == 3 else "(H, W)"))
        offs = np.concatenate([[0], np.cumsum([a.size for a in arrays])]).astype(np.int64)
        flat = np.empty(int(offs[-1]), np.uint8)
        for a, o in zip(arrays, offs):
            flat[o:o + a.size] = a.reshape(-1)
        return flat, offs[:-1], [a.shape[:2] for a in arrays]

    def apply(self, images, labels, params):
        B, S, s = len(images), self.crop_size, self.reduced_size
        p = np.asarray(params)
        if B < 1 or len(labels) != B or p.shape != (B, len(_lib.IRN_BATCH_PARAMS)) or p.dtype.kind not in "iu":
            raise ValueError("TrainBatcher.apply: %d images, %d labels, params %r %s" % (B, len(labels), p.shape, p.dtype))
        img, ioff, sizes = self._pack("image", images, 3)
        lab, loff, lsizes = self._pack("label", labels, 2)
        if sizes != lsizes:
            raise ValueError("TrainBatcher.apply: the labels' sizes %r are not the images' %r" % (lsizes[:4], sizes[:4]))
        if self.outsize is not None and any((int(r[0]), int(r[1])) != self.outsize for r in p):
            raise ValueError("TrainBatcher.apply: a record resizes to another size than outsize %r" % (self.outsize,))
        outs, held = [], []
        try:
            held.append(DeviceMaps.from_host(self.ctx, img))
            held.append(DeviceMaps.from_host(self.ctx, lab))
            outs.append(DeviceMaps(self.ctx, (B, 3, S, S), np.float32))
            outs.append(DeviceMaps(self.ctx, (B, S, S), np.uint8))
            outs.append(DeviceMaps(self.ctx, (B, s, s), np.uint8))
            _lib.irn_train_batch(self.ctx, held[0].ptr, held[1].ptr, sizes, ioff, loff, p, S, self.norm.mean, self.norm.std, self.pre_div255,
                                 self.stage, outs[0].ptr, outs[1].ptr, outs[2].ptr)
            return tuple(outs)
        except Exception:
            for m in outs:
                m.free()
            raise
        finally:
            for m in held:  # (pooled: reuse is ordered behind the launches on the context's stream)
                m.free()


class IrnTrainer(TrainerCore):
    """One IRNet training step after another, and the closing pass: step/train_irn.py:86-90, 105-164 on the device.

        IrnTrainer(model, path_index, lr, weight_decay, max_step, power=0.9, sgd_momentum=None, valid_below=21)
          model         an EdgeDisplacement wrapper with its state dict loaded; the trainer trains ITS net in place
          lr, weight_decay, max_step, power, sgd_momentum    PolyOptimizer's (misc.torchutils: power is upstream's `momentum`
                        argument, the poly exponent; sgd_momentum None = the value of weight_decay, the upstream behaviour)
    The parameters and the momentum are two resident float32 DeviceMaps of irn_grad().grad_elems floats in the layout of IrnGrads,
    initialised from the model's state dict and zeros; a step never downloads them.

    step(x, label) -> losses   AffinityLoss.grad_step, wsc_irn_sgd_step at the schedule's two rates, wsc_net_irn_load_params:
                    afterwards the net computes with the updated heads.  Downloads the loss values and nothing else; everything
                    it allocates is freed on every path.
    global_step, lr             the optimiser's step count and the (edge, dp) rates of the NEXT step
    params_host() / momentum_host()   {name: array in torch's shape}
    fit_dp_mean(batches) -> float32 (2,)   the closing loop: per batch (x (N,3,S,S), plain samples) forward_train_dev, the
                    per-channel mean of dp_out over (N, H, W) in double minus the net's current mean shift (eval-mode MeanShift
                    subtracts running_mean) into slot i of a device array; ONE download of the [n_batches][2] doubles at the
                    end, their mean in double rounded to float32, installed in the net (wsc_net_set_mean_shift)
    state_dict()    the model's full state dict with the updated head tensors and mean_shift.running_mean; also refreshes the
                    wrapper's own copy, so the trained model and a fresh one loaded from the dict behave identically
    save(path) / IrnTrainer.load(path, model, path_index, ...)   np.save / np.load(...).item() of state_dict() with the momentum
                    under "__momentum__" and the step count under "__step__"
    close() / a context manager releases the two buffers (the model stays the caller's)"""

    def __init__(self, model, path_index, lr, weight_decay, max_step, power=0.9, sgd_momentum=None, valid_below=21, ctx=None):
        self.model = model
        self.ctx = model.ctx
        if ctx is not None and ctx is not self.ctx:
            raise ValueError("IrnTrainer: the model lives on another context")
        self.loss = AffinityLoss(path_index, valid_below=valid_below, ctx=self.ctx)
        self.grad = model.irn_grad()
        self.opt = PolyOptimizer(self.grad, lr, weight_decay, max_step, momentum=power, sgd_momentum=sgd_momentum)
        self._init_buffers(lambda: self.grad.flat_params(model._sd))

    def _fields(self):
        return _lib.IrnGrad.fields(self.grad.layout)

    def _grad_now(self):
        return self.model.irn_grad()

    @property
    def global_step(self):
        return self.opt.global_step

    @property
    def lr(self):
        return self.opt.lr_now()

    def step(self, x, label):
        self._live()
        losses, grads = self.loss.grad_step(self.model, x, label)
        try:
            self.opt.step(self.params, grads.maps, self.mom)
            self.grad.load_params(self.params.ptr)
        finally:
            grads.free()
        return losses

    def fit_dp_mean(self, batches, n_batches=None):
        """n_batches: the count of an iterable that is consumed one batch at a time (step.train_irn: each batch is a DeviceMaps
        that lives only until the next one is asked for); None: `batches` is listed first"""
        self._live()
        if n_batches is None:
            batches = list(batches)
            n_batches = len(batches)
        n_batches = int(n_batches)
        if n_batches < 1:
            raise ValueError("IrnTrainer.fit_dp_mean: no batches")
        net = self.model._ensure_net()
        shift = net.get_mean_shift()
        with DeviceMaps(self.ctx, (n_batches, 2), np.float64) as slots:
            seen = 0
            for i, x in enumerate(batches):
                if i >= n_batches:
                    raise ValueError("IrnTrainer.fit_dp_mean: more than the %d batches announced" % n_batches)
                edge, dp = self.model.forward_train_dev(x)
                with edge, dp:
                    N, C, Hd, Wd = dp.shape
                    _lib.channel_mean_nchw(self.ctx, dp.ptr, N, C, Hd, Wd, slots.ptr + 16 * i, sub=shift)
                seen = i + 1
            if seen != n_batches:
                raise ValueError("IrnTrainer.fit_dp_mean: %d batches, %d announced" % (seen, n_batches))
            means = slots.to_host()  # the pass's one download
        mean = (means.sum(axis=0) / n_batches).astype(np.float32)
        net.set_mean_shift(mean)
        self.model._sd["mean_shift.running_mean"] = mean.copy()
        return mean

    def state_dict(self):
        self._live()
        sd = self.model._sd
        sd.update(self.params_host())
        sd["mean_shift.running_mean"] = self.model._ensure_net().get_mean_shift()
        return {k: v.copy() for k, v in sd.items()}

    _params_dict = state_dict

    def _step_dict(self):
        return {"global_step": self.global_step}

    def _set_step(self, step):
        self.opt.global_step = int(step.get("global_step", 0))

    @classmethod
    def load(cls, path, model, path_index, lr, weight_decay, max_step, **kwargs):
        tensors, marked = cls._read(path)
        model.load_state_dict(tensors)
        model.cuda()
        return cls(model, path_index, lr, weight_decay, max_step, **kwargs)._resume(marked)
