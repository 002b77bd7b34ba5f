"""Modified-VGG16 CAM network -- mirror of 03b_irn/net/vgg16_cam.py (CAM.forward :24-60) on
net/vgg16.py:44 + common_cnn.make_layers :128-141.  Weights: a torch-style state_dict with keys
`vgg16.layer<L>.<idx>.{weight,bias,...}`, `vgg16.classifier.0.{weight,bias}` and `thresholds`
(what common_cnn._load_pretrained leaves in the module after transplanting the Keras .h5/.mat,
common_cnn.py:25-82).

`pooling`: the geometry of the three MaxPooling2D layers when it is not the torch port's MaxPool2d(2, 2) -- a list of
(k, stride, 'same' | 'valid') in the order the pools occur, as keras_store.read_architecture takes it from a session's
architecture file; None is the fixed architecture."""
import numpy as np

from .. import _lib
from ..device import DeviceMaps, device_input
from .common import DeviceCAMBase, normalize_pooling

ADP_INDS_X17 = [2, 3, 4, 6, 7, 8, 9, 12, 13, 14, 16, 17, 18, 21, 22, 23, 25, 26, 28, 29, 30, 32, 33, 35, 37, 38, 40,
                45, 48, 49, 50]  # common_cam.py:26-29


class CAM(DeviceCAMBase):
    arch = _lib.ARCH_VGG16_CAM
    root = "vgg16"

    def __init__(self, model_dir=None, dataset="voc12", tag="", num_classes=20, use_cls=None, precision=None, *, pooling=None):
        super().__init__(num_classes, precision)
        self.pooling = normalize_pooling(pooling)
        self.model_dir = model_dir
        self.dataset = dataset
        self.tag = tag
        self.use_cls = use_cls
        self.thresholds = 0.5 * np.ones(num_classes, dtype=np.float32)  # common_cnn.py:22
        self.batchnorm = self._has_batchnorm()
        if model_dir is not None and tag:
            self._load_pretrained(model_dir, tag)

    def _has_batchnorm(self):
        return self.dataset not in ("adp_morph", "adp_func")  # vgg16_cam.py:16-19: the ADP VGG16 models carry no BatchNorm

    def set_pooling(self, spec):
        """The pools' geometry (see the module docstring); the packed nets built for the previous one are released."""
        self.pooling = normalize_pooling(spec)
        self._release_net()
        for net in self.__dict__.pop("_gradcam_nets", {}).values():
            net.close()
        return self

    def _load_pretrained(self, model_dir, tag):
        """CommonCNN._load_pretrained (common_cnn.py:25-41): Keras <tag>.h5 + <tag>.mat under <model_dir>/<tag>/.
        When the files are absent the wrapper stays empty until load_state_dict() is called (the reference would
        raise at construction; make_cam.run passes `args.state_dict` for weightless dry runs)."""
        import os

        from .common import load_pretrained

        if os.path.exists(os.path.join(model_dir, tag, tag + ".h5")):
            self.load_state_dict(load_pretrained(model_dir, tag, self.root, self.batchnorm), strict=True)

    def load_state_dict(self, state_dict, strict=True):
        super().load_state_dict(state_dict, strict)
        if "thresholds" in self._sd:
            self.thresholds = np.asarray(self._sd.pop("thresholds"), dtype=np.float32)
        return self

    # ---- 01_train: the stack in training mode (wsc_net_forward_cls_train / wsc_net_backward_cls) --------------------------------
    def _release_net(self):
        grad = self.__dict__.pop("_cls_grad", None)
        if grad is not None:
            grad.close()
        run = self.__dict__.pop("_bn_running", None)
        if run is not None:
            run.free()
        super()._release_net()

    def bn_keys(self):
        """The state-dict prefixes of the stack's BatchNorm layers in stack order ([] for a net without)."""
        from .common import plain_module_order

        return [key for kind, key in plain_module_order(self.root, True) if kind == "bn" and key + ".running_mean" in self._sd]

    def bn_running_dev(self):
        """The running statistics forward_train_dev updates: one float32 DeviceMaps, per BatchNorm layer in stack order its
        running mean then its running variance; created from the state dict on first use, released with the net.  None for a net
        without BatchNorm."""
        self._ensure_net()
        if getattr(self, "_bn_running", None) is None:
            keys = self.bn_keys()
            if not keys:
                return None
            flat = np.concatenate([self._sd[k + "." + n].reshape(-1) for k in keys for n in ("running_mean", "running_var")])
            self._bn_running = DeviceMaps.from_host(self._ctx, flat, dtype=np.float32)
        return self._bn_running

    def bn_running(self):
        """{'<bn>.running_mean' / '<bn>.running_var': array}: the running statistics as forward_train_dev left them"""
        run, out, at = self.bn_running_dev(), {}, 0
        flat = run.to_host() if run is not None else None
        for k in self.bn_keys():
            for n in ("running_mean", "running_var"):
                c = self._sd[k + "." + n].size
                out[k + "." + n] = flat[at:at + c].copy()
                at += c
        return out

    def classifier_params(self, num_classes=None):
        """(weight (C, F), bias (C,) or None) of the classifier's Linear, the rows the device net uses"""
        C = self.num_classes if num_classes is None else int(num_classes)
        bias = self._sd.get(self.root + ".classifier.0.bias")
        return self._sd[self.root + ".classifier.0.weight"][:C], None if bias is None else bias[:C]

    def cls_grad(self):
        """The _lib.ClsGrad of the model's net (created on first use, released with the net)."""
        net = self._ensure_net()
        if getattr(self, "_cls_grad", None) is None:
            self._cls_grad = _lib.ClsGrad(net, self._extra_tensors(self._sd))
        return self._cls_grad

    def forward_train_dev(self, x, keep=True, bn_keep=0.99, dropout=None):
        """The stack in training mode (make_layers' conv -> ReLU -> BatchNorm on the BATCH statistics): x float32 (B, 3, H, W), a
        host array / tensor or a device.DeviceMaps of the model's context (read in place) -> (feat DeviceMaps (B, h, w, F), the
        map ClsLoss reads, tape): the cls_train.ClsTape backward_dev needs; the caller frees both.  keep=False: feat alone.
        dropout: None (the `D` entries of the table are the identity: wsc_net_forward_cls_train), or (drop_prob, seed, step) --
        the shape SegNet.forward_dev takes -- for wsc_net_forward_cls_train_drop: the sites active under the project's own
        counter-based keep-masks of (seed, step, site, element index) (not Keras' random stream).  VGG16:
        behind both entries of layer5; feat is the dropped output of the second.  M7: behind layer3_p2, and feat is then the
        POOLED, dropped map (B, hp, wp, F) whose global max ClsLoss takes.  The reference's models use 0.5.  The tape records the
        triple for backward_dev; needs keep=True.
        bn_keep: the weight of the OLD running value in the update of the running statistics (bn_running_dev), Keras' `momentum`:
        BatchNormalization(momentum=0.99) is 0.99.  torch's nn.BatchNorm2d(momentum=m) weighs the NEW value with m, so the torch
        port's BatchNorm2d(v, eps=0.001, momentum=0.99) is bn_keep = 0.01.  The batch variance enters unbiased (M / (M - 1)), as
        in torch and TensorFlow's fused batch norm; Keras 2.2's own factor is unpinned.  None: the running statistics stay."""
        from ..cls_train import ClsTape

        if dropout is not None and not keep:
            raise ValueError("forward_train_dev: dropout=%r needs keep=True (the backward pass needs the triple the tape records)" % (dropout,))
        net = self._ensure_net()
        ctx = self._ctx
        xd, mine = device_input(ctx, x, np.float32, "forward_train_dev")
        feat = tape = None
        try:
            if len(xd.shape) != 4 or xd.shape[1] != 3 or 0 in xd.shape:
                raise ValueError("forward_train_dev: x has shape %r, expected (B, 3, H, W)" % (xd.shape,))
            if bn_keep is not None and not 0.0 <= float(bn_keep) <= 1.0:
                raise ValueError("forward_train_dev: bn_keep = %r (the weight of the old running value, 0 .. 1)" % (bn_keep,))
            B, H, W = xd.shape[0], xd.shape[2], xd.shape[3]
            if dropout is not None:
                drop_prob, seed, step = float(dropout[0]), int(dropout[1]), int(dropout[2])
            h, w = net.cam_size_hw(H, W) if dropout is None else net.cls_feat_dims(H, W, drop_prob > 0)
            run = None if bn_keep is None else self.bn_running_dev()
            entries, elems = net.cls_tape_plan(B, H, W)
            feat = DeviceMaps(ctx, (B, h, w, net.feat_channels()), np.float32)
            tape = ClsTape(DeviceMaps(ctx, (elems,), np.float32), entries, B, H, W,
                           None if dropout is None else (drop_prob, seed, step))
            if dropout is None:
                net.forward_cls_train(xd.ptr, B, H, W, tape.maps.ptr, elems, feat.ptr, keep=0.0 if bn_keep is None else bn_keep,
                                      run_dev=None if run is None else run.ptr)
            else:
                net.forward_cls_train_drop(xd.ptr, B, H, W, tape.maps.ptr, elems, feat.ptr, B * h * w * net.feat_channels(), drop_prob,
                                           seed, step, keep=0.0 if bn_keep is None else bn_keep, run_dev=None if run is None else run.ptr)
            if keep:
                return feat, tape
            tape.free()
            return feat
        except Exception:
            for m in (feat, tape):
                if m is not None:
                    m.free()
            raise
        finally:
            if mine is not None:
                mine.free()

    def backward_dev(self, tape, dfeat):
        """The backward pass of the stack (wsc_net_backward_cls): the tape of forward_train_dev and d loss / d feat (B, h, w, F) or
        (B, h w, F) float32, a DeviceMaps of the model's context (HeadGrads.feat of ClsLoss.grad_step), read in place ->
        cls_train.ClsGrads (the caller frees it).  The chain rule evaluated at the tape, in exact fp32 whatever the net's precision.
        A tape of forward_train_dev(dropout=(drop_prob, seed, step)) carries the triple: wsc_net_backward_cls_drop regenerates
        the masks from it, and dfeat has the shape of that pass's feat (M7: the pooled (B, hp, wp, F))."""
        from ..cls_train import ClsGrads, ClsTape

        net = self._ensure_net()
        ctx = self._ctx
        if not isinstance(tape, ClsTape) or tape.maps.ptr is None or tape.maps.ctx is not ctx:
            raise ValueError("backward_dev: tape is no live ClsTape of the model's context")
        if not isinstance(dfeat, DeviceMaps) or dfeat.dtype != np.float32 or dfeat.ctx is not ctx or dfeat.ptr is None:
            raise ValueError("backward_dev: dfeat is no live float32 DeviceMaps of the model's context")
        drop = getattr(tape, "dropout", None)
        h, w = net.cam_size_hw(tape.H, tape.W) if drop is None else net.cls_feat_dims(tape.H, tape.W, drop[0] > 0)
        F = net.feat_channels()
        if tuple(dfeat.shape) not in ((tape.B, h, w, F), (tape.B, h * w, F)):
            raise ValueError("backward_dev: dfeat has shape %r, expected %r" % (tuple(dfeat.shape), (tape.B, h, w, F)))
        grad = self.cls_grad()
        out = DeviceMaps(ctx, (grad.grad_elems,), np.float32)
        try:
            if drop is None:
                grad.backward(tape.B, tape.H, tape.W, tape.maps.ptr, tape.elems, dfeat.ptr, out.ptr)
            else:
                grad.backward_drop(tape.B, tape.H, tape.W, tape.maps.ptr, tape.elems, dfeat.ptr, tape.B * h * w * F, out.ptr, *drop)
        except Exception:
            out.free()
            raise
        return ClsGrads(out, grad.layout)

    def load_params_dev(self, flat):
        """The net rewritten in place from a flat parameter buffer in cls_grad().param_layout (wsc_net_cls_load_params): `flat` a
        host array of param_elems floats (uploaded once) or a float32 DeviceMaps of the model's context (read in place).  The
        packed conv rows, BatchNorm's gamma / beta and its inference fold -- from bn_running_dev(), the running statistics as
        forward_train_dev left them --, the classifier and VGG16's CAM head afterwards have the bits of a model created from the
        same floats and statistics; an M7 head, the Grad-CAM alpha, is no parameter and stays.  The wrapper's state dict is NOT
        touched (cls_train.ClsTrainer.state_dict downloads).  The model's cached gradcam_net()s hold packed copies of the old
        weights: they are released."""
        self._ensure_net()
        ctx, grad = self._ctx, self.cls_grad()
        fd, mine = device_input(ctx, flat, np.float32, "load_params_dev")
        try:
            if int(np.prod(fd.shape)) != grad.param_elems:
                raise ValueError("load_params_dev: %d floats, the layout has %d" % (int(np.prod(fd.shape)), grad.param_elems))
            run = self.bn_running_dev()
            grad.load_params(fd.ptr, None if run is None else run.ptr)
        finally:
            if mine is not None:
                mine.free()  # (pooled: reuse is ordered behind the launches on the context's stream)
        for net in self.__dict__.pop("_gradcam_nets", {}).values():
            net.close()
        return self

    def predict_labels(self, score):
        """vgg16_cam.py:37-45: score >= thresholds; if nothing passes on non-ADP data force argmax."""
        y = score >= self.thresholds[:len(score)]
        if self.dataset not in ("adp_morph", "adp_func") and y.sum() == 0:
            y[np.argmax(score)] = True
        if "X1.7" in self.tag:
            y = y[ADP_INDS_X17]
        return y

    # ---- ADP background / other-tissue channels: common_cam.py:31-92, on the device --------------------------
    def adp_channel_lists(self):
        """(mode, use, adipose, exceptions) as channel indices of the network's CAM stack: mode 0 = adp_morph
        (_adp_modify_morph :31-55), 1 = adp_func (_adp_modify_func :57-92); the X1.7 class filter (:26-29, applied to the
        CAM before the modification, vgg16_cam.py:49-50) is composed into the lists."""
        filt = ADP_INDS_X17 if "X1.7" in self.tag else list(range(self.num_classes))
        use = [filt[int(i)] for i in self.use_cls]
        return (0 if self.dataset == "adp_morph" else 1), use, [filt[i] for i in (18, 19, 20)], [filt[i] for i in (28, 29, 30)]

    def adp_out_channels(self):
        return len(self.use_cls) + (1 if self.dataset == "adp_morph" else 2)

    def adp_modify_device(self, ctx, cam_dev, B, n_sc, h, w, origs, out_dev=None, stage=None):
        """The ADP map stacks of a device batch (vgg16_cam.py:51-58), never leaving the GPU:
        0.75 * expit(4 * (mean_rgb - 240)) of every ORIGINAL (un-normalised, un-flipped) image, Gaussian smoothed (sigma 2),
        cv2-bilinear resized to the CAM grid (wsc_hsn_background), then the background / 'other' channels joined with the
        use_cls CAM channels and summed over the scales (wsc_cam_adp_modify).
          cam_dev float32 [B][n_sc][C][h][w];  origs: B * n_sc uint8 (H0, W0, 3) arrays in (image, scale) order;
          stage: optional (PinnedBuffer, DeviceBuffer) pair of >= sum(H0 W0 3) bytes for an asynchronous upload.
        -> (out_dev float32 [B][Cout][h][w], Cout)."""
        origs = [np.ascontiguousarray(o, dtype=np.uint8) for o in origs]
        assert len(origs) == B * n_sc and all(o.ndim == 3 and o.shape[2] == 3 for o in origs)
        offs = np.concatenate(([0], np.cumsum([o.size for o in origs]))).astype(np.int64)
        total = int(offs[-1])
        if stage is not None:
            pin, rgb_dev = stage
            buf = pin.view((total,), np.uint8)
            for k, o in enumerate(origs):
                buf[offs[k]:offs[k + 1]] = o.reshape(-1)
            ctx.h2d_async(rgb_dev, pin, total)
        else:
            rgb_dev = ctx.to_device(np.concatenate([o.reshape(-1) for o in origs]), pooled=True)
        hw = h * w
        bg_dev = ctx.alloc(B * n_sc * hw * 8, pooled=True)
        k = 0
        while k < len(origs):  # runs of equal size (ADP patches all are 272 x 272: one call)
            e = k + 1
            while e < len(origs) and origs[e].shape == origs[k].shape:
                e += 1
            H0, W0 = origs[k].shape[:2]
            _lib.hsn_background(ctx, rgb_dev.ptr + int(offs[k]), e - k, H0, W0, bg_dev.ptr + k * hw * 8, out_hw=(h, w))
            k = e
        mode, use, adip, exc = self.adp_channel_lists()
        Cout = len(use) + 1 + mode
        if out_dev is None:
            out_dev = ctx.alloc(B * Cout * hw * 4, pooled=True)
        _lib.cam_adp_modify(ctx, cam_dev, B, n_sc, self.num_classes, hw, bg_dev, mode, use, adip, exc, out_dev)
        bg_dev.free()  # pooled: reused in stream order
        if stage is None:
            rgb_dev.free()
        return out_dev, Cout

    def forward(self, x, x_orig=None):
        """-> (cam (C,h,w), y bool (C,)) as vgg16_cam.py:24-60 / m7_cam.py:22-57; for the ADP datasets
        `x_orig` is the (2,H0,W0,3) uint8 image pair of the ADP dataloader."""
        assert (self.dataset in ("adp_morph", "adp_func")) ^ (x_orig is None)
        is_torch = hasattr(x, "detach")
        xn = x.detach().cpu().numpy() if is_torch else np.asarray(x)
        if x_orig is None:
            cam, score = self.forward_batch(xn[None], want_score=True)
            cam = cam[0]
            if "X1.7" in self.tag:
                cam = cam[ADP_INDS_X17]
        else:  # the ADP channels are synthesised on the device, between the CAM head and the copy out
            x_orig = x_orig.detach().cpu().numpy() if hasattr(x_orig, "detach") else np.asarray(x_orig)
            net = self._ensure_net()
            ctx = self._ctx
            xc = np.ascontiguousarray(xn[None], dtype=np.float32)
            S = xc.shape[-1]
            h = net.cam_size(S)
            x_dev = ctx.to_device(xc, pooled=True)
            cam_dev = ctx.alloc(self.num_classes * h * h * 4, pooled=True)
            score_dev = ctx.alloc(self.num_classes * 4, pooled=True)
            net.forward_cam(x_dev, 1, S, cam_dev, score_dev)
            out_dev, Cout = self.adp_modify_device(ctx, cam_dev, 1, 1, h, h, [x_orig[0]])
            cam = ctx.to_host(out_dev, (Cout, h, h), np.float32)
            score = ctx.to_host(score_dev, (1, self.num_classes), np.float32)
            for b in (x_dev, cam_dev, score_dev, out_dev):
                b.free()
        y = self.predict_labels(score[0])
        if is_torch:
            import torch

            return torch.from_numpy(cam), torch.from_numpy(y)
        return cam, y

    __call__ = forward
