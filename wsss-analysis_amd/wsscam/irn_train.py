"""03b_irn/step/train_irn.py on libwsscam: the loss of one training step and the gradient it sends into the two head outputs.

    AffinityLoss   AffinityDisplacementLoss.forward's four loss tensors (net/resnet50_irn.py:198-213), the pair labels the
                   affinity datasets attach (GetAffinityLabelFromIndices, voc12/dataloader.py:115-131) and the reductions of
                   step/train_irn.py:114-125 in one device call (wsc_irn_aff_loss; the formulas, the tie rules and the double
                   arithmetic: include/wsscam.h), with d total / d edge_out and d total / d dp_out.  loss_step chains it behind
                   EdgeDisplacement.forward_train_dev (Net.forward in training mode).
    reduce_label   the IR label at the resolution of the head outputs (voc12/dataloader.py:317)

The backward pass of the heads (GroupNorm, 1x1 conv, bilinear upsample), PolyOptimizer, the affinity datasets' augmentation and
the closing dp_mean pass are not here."""
import numpy as np

from . import _lib
from .misc import imutils
from .secdsrg import DeviceMaps


def reduce_label(label):
    """imutils.pil_rescale(label, 0.25, 0) (voc12/dataloader.py:317, and the ADP / DeepGlobe twins): the (H, W) uint8 IR label
    of cam_to_ir_label, nearest-neighbour, at a quarter of the crop -- the resolution of edge_out and dp_out."""
    label = np.asarray(label)
    if label.ndim != 2:
        raise ValueError("reduce_label: label has shape %r, expected (H, W)" % (label.shape,))
    return np.ascontiguousarray(imutils.pil_rescale(label.astype(np.uint8), 0.25, 0))


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
        """-> DeviceMaps of `dtype`; shape: a tuple to match, or a function that says whether the shape fits"""
        if isinstance(a, DeviceMaps):
            if a.dtype != np.dtype(dtype):
                raise ValueError("AffinityLoss: %s is %s on the device, not %s" % (name, a.dtype, np.dtype(dtype)))
        else:
            a = np.asarray(a)
            if a.dtype.kind not in "fiub":
                raise ValueError("AffinityLoss: %s has dtype %s, not a real number type" % (name, a.dtype))
        got = tuple(a.shape)
        if not (shape(got) if callable(shape) else got == tuple(shape)):
            raise ValueError("AffinityLoss: %s has shape %r%s" % (name, got, "" if callable(shape) else ", expected %r" % (tuple(shape),)))
        if isinstance(a, DeviceMaps):
            return a
        held.append(DeviceMaps.from_host(self.ctx, a, dtype=dtype))
        return held[-1]

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

    def loss_step(self, net, x, label, want_grad=True):
        """One training step up to the gradient of the head outputs: net.forward_train_dev(x) (an EdgeDisplacement wrapper; x
        (B, 3, S, S)), then this loss on its outputs -> (losses, grad_edge, grad_dp, edge_out, dp_out), the last four DeviceMaps
        the caller frees (the gradients None when want_grad is false).  `net` must live on this loss's context."""
        if net.ctx is not self.ctx:
            raise ValueError("AffinityLoss.loss_step: the network lives on another context than the loss")
        edge, dp = net.forward_train_dev(x)
        try:
            if edge.shape[1:] != dp.shape[2:]:
                raise ValueError("AffinityLoss.loss_step: edge_out is %r and dp_out %r: the loss needs one resolution" % (edge.shape, dp.shape))
            losses, g_edge, g_dp = self(edge, dp, label, want_grad=want_grad)
        except Exception:
            edge.free()
            dp.free()
            raise
        return losses, g_edge, g_dp, edge, dp
