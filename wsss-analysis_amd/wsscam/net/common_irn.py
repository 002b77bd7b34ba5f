"""Shared host logic of the IRNet EdgeDisplacement wrappers (03b_irn/net/*_irn.py, class EdgeDisplacement)."""
import numpy as np

from .. import _lib
from ..device import DeviceMaps, device_input
from .common import DeviceCAMBase


class EdgeDisplacementBase(DeviceCAMBase):
    """EdgeDisplacement.forward (resnet50_irn.py:218-232, vgg16_irn.py:308-321): x (2,3,h,w) [orig, h-flip] is
    zero-padded on the right / bottom to crop_size, run through the backbone + edge / displacement heads,
    cropped to the stride-4 feature size, and returns (edge (1? no: (fh,fw) as edge_out[0]/2 + edge_out[1].flip(-1)/2
    has shape (1,fh,fw)), dp (2,fh,fw))."""

    def __init__(self, num_classes, crop_size=512, stride=4, precision=None):
        super().__init__(num_classes, precision)
        self.crop_size = crop_size
        self.stride = stride
        self._irn_grad = None  # the _lib.IrnGrad of the net (irn_grad())

    def forward_batch(self, x):
        """x: numpy/torch float32 (B,2,3,h,w) -> (edge (B,1,fh,fw), dp (B,2,fh,fw)) numpy."""
        edge_dev, dp_dev, (B, fh, fw) = self.forward_batch_device(x)
        ctx = self._ctx
        return ctx.to_host(edge_dev, (B, 1, fh, fw), np.float32), ctx.to_host(dp_dev, (B, 2, fh, fw), np.float32)

    def forward_batch_device(self, x, ctx=None, chain=None):
        """forward_batch with the outputs left in HBM: (edge_dev float32 [B][fh][fw], dp_dev [B][2][fh][fw], (B, fh, fw)).
        x: (B,2,3,h,w) array / tensor, or a list of B (2,3,h,w) arrays of one size (copied straight into the page-locked,
        zero-padded staging batch: no stacked temporary, no pageable upload).  `ctx`: run on this context (a lane of the
        make_sem_seg_labels driver: its own stream, staging batch and workspace) instead of the model's own; `chain`: that
        driver's _lib.StackChain (the lanes' network passes take turns on the device)."""
        net = self._ensure_net()
        if isinstance(x, (list, tuple)):
            items = [np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32) for v in x]
        else:
            xn = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
            assert xn.ndim == 5, xn.shape
            items = list(np.asarray(xn, dtype=np.float32))
        B = len(items)
        assert B > 0 and all(v.shape == items[0].shape and v.ndim == 4 and v.shape[:2] == (2, 3) for v in items), \
            [v.shape for v in items][:4]
        h, w = items[0].shape[2], items[0].shape[3]
        S = self.crop_size
        if h > S or w > S:
            raise ValueError("input %dx%d is larger than crop_size %d" % (h, w, S))
        fh, fw = (h - 1) // self.stride + 1, (w - 1) // self.stride + 1
        ctx = ctx or self._ctx
        st = self.__dict__.setdefault("_stage", {}).setdefault(id(ctx), {})
        if st.get("key") != (B, S):  # page-locked (B,2,3,S,S) staging batch + its device twin, kept across calls
            for k in ("pin", "dev"):
                if st.get(k) is not None:
                    st[k].free()
            st.update(key=(B, S), pin=ctx.host_alloc(B * 2 * 3 * S * S * 4), dev=ctx.alloc(B * 2 * 3 * S * S * 4), hw=None)
        xp = st["pin"].view((B, 2, 3, S, S), np.float32)
        ctx.sync()  # the previous batch's upload has left the staging buffer
        if st["hw"] != (h, w):
            xp[...] = 0.0  # F.pad(x, [0, S - w, 0, S - h]): the margins stay zero while the image size does not change
            st["hw"] = (h, w)
        for i, v in enumerate(items):
            xp[i, :, :, :h, :w] = v
        ctx.h2d_async(st["dev"], st["pin"], B * 2 * 3 * S * S * 4)
        edge_dev = ctx.alloc(B * fh * fw * 4, pooled=True)
        dp_dev = ctx.alloc(B * 2 * fh * fw * 4, pooled=True)
        if chain is not None:  # (a driver with several batches in flight: one conv stack at a time, _lib.StackChain)
            chain.run(ctx, lambda: net.forward_edge(st["dev"], B, S, fh, fw, edge_dev, dp_dev, ctx=ctx))
        else:
            net.forward_edge(st["dev"], B, S, fh, fw, edge_dev, dp_dev, ctx=ctx)
        return edge_dev, dp_dev, (B, fh, fw)

    def forward_train_dev(self, x, keep=False):
        """Net.forward in training mode (resnet50_irn.py:110-133, what AffinityDisplacementLoss.forward calls at :200), outputs
        left in HBM: x float32 (N,3,S,S), a host array / tensor or a device.DeviceMaps of the model's context (read in place)
        -> (edge_out DeviceMaps (N,He,We), dp_out DeviceMaps (N,2,Hd,Wd)): plain samples, no flip pairing, no crop, no mean shift
        (MeanShift is the identity while training), no sigmoid.  keep=True: (edge_out, dp_out, tape) -- the same launches and
        bits, and the tape backward_dev needs (an irn_train.EdgeTape; the caller frees it)."""
        from ..irn_train import EdgeTape

        net = self._ensure_net()
        ctx = self._ctx
        xd, mine = device_input(ctx, x, np.float32, "forward_train_dev")
        edge = dp = tape = None
        try:
            if len(xd.shape) != 4 or xd.shape[1] != 3 or xd.shape[2] != xd.shape[3] or 0 in xd.shape:
                raise ValueError("forward_train_dev: x has shape %r, expected (N, 3, S, S)" % (xd.shape,))
            N, S = xd.shape[0], xd.shape[2]
            (He, We), (Hd, Wd) = net.edge_size(S)
            edge = DeviceMaps(ctx, (N, He, We), np.float32)
            dp = DeviceMaps(ctx, (N, 2, Hd, Wd), np.float32)
            if not keep:
                net.forward_edge_raw(xd.ptr, N, S, edge.ptr, dp.ptr)
                return edge, dp
            entries, elems = net.edge_tape_plan(N, S)
            tape = EdgeTape(DeviceMaps(ctx, (elems,), np.float32), entries, N, S)
            net.forward_edge_tape(xd.ptr, N, S, tape.maps.ptr, elems, edge.ptr, dp.ptr)
            return edge, dp, tape
        except Exception:
            for m in (edge, dp, tape):
                if m is not None:
                    m.free()
            raise
        finally:
            if mine is not None:
                mine.free()

    def _release_net(self):
        grad = getattr(self, "_irn_grad", None)
        if grad is not None:  # (it holds kernels packed from the net's weights: it goes first)
            grad.close()
            self._irn_grad = None
        super()._release_net()

    def irn_grad(self):
        """The _lib.IrnGrad of the model's net (created on first use, released with the net)."""
        net = self._ensure_net()
        if getattr(self, "_irn_grad", None) is None:
            self._irn_grad = _lib.IrnGrad(net, self._extra_tensors(self._sd))
        return self._irn_grad

    def load_params_dev(self, flat):
        """wsc_net_irn_load_params: the heads' packed weights and GroupNorm vectors, the two final convs and the data-gradient
        kernels of the backward pass rewritten on the device from `flat`, float32 (grad_elems,) in the layout of IrnGrads -- a
        DeviceMaps of the model's context (read in place), or a host array (uploaded once; irn_grad().flat_params(sd) makes one).
        Afterwards the net has the bits of a model loaded with those head tensors.  The wrapper's own state dict is not touched
        (irn_train.IrnTrainer.state_dict does both)."""
        g = self.irn_grad()
        fd, mine = device_input(self._ctx, flat if isinstance(flat, DeviceMaps) else np.asarray(flat).reshape(-1), np.float32, "load_params_dev")
        try:
            if fd.shape != (g.grad_elems,):
                raise ValueError("load_params_dev: %r must be (%d,), the layout's size" % (fd.shape, g.grad_elems))
            g.load_params(fd.ptr)
        finally:
            if mine is not None:
                mine.free()

    def backward_dev(self, tape, grad_edge, grad_dp):
        """total_loss.backward() through the heads (train_irn.py:127; the backbone stages are detached): tape of
        forward_train_dev(x, keep=True), grad_edge (N,He,We) or (N,1,He,We) and grad_dp (N,2,Hd,Wd) float32 DeviceMaps of the
        model's context (what AffinityLoss hands out), read in place -> irn_train.IrnGrads (the caller frees it)."""
        from ..irn_train import EdgeTape, IrnGrads

        net = self._ensure_net()
        ctx = self._ctx
        if not isinstance(tape, EdgeTape) or tape.maps.ptr is None or tape.maps.ctx is not ctx:
            raise ValueError("backward_dev: tape is no live EdgeTape of the model's context")
        (He, We), (Hd, Wd) = net.edge_size(tape.S)
        for name, m, shapes in (("grad_edge", grad_edge, ((tape.N, He, We), (tape.N, 1, He, We))), ("grad_dp", grad_dp, ((tape.N, 2, Hd, Wd),))):
            if not isinstance(m, DeviceMaps) or m.dtype != np.float32 or m.ctx is not ctx or m.ptr is None:
                raise ValueError("backward_dev: %s is no live float32 DeviceMaps of the model's context" % name)
            if tuple(m.shape) not in shapes:
                raise ValueError("backward_dev: %s has shape %r, expected %r" % (name, tuple(m.shape), shapes[0]))
        grad = self.irn_grad()
        out = DeviceMaps(ctx, (grad.grad_elems,), np.float32)
        try:
            net.backward_edge(grad, tape.N, tape.S, tape.maps.ptr, tape.elems, grad_edge.ptr, grad_dp.ptr, out.ptr)
        except Exception:
            out.free()
            raise
        return IrnGrads(out, grad.layout)

    def forward(self, x):
        is_torch = hasattr(x, "detach")
        xn = x.detach().cpu().numpy() if is_torch else np.asarray(x)
        edge, dp = self.forward_batch(xn[None])
        if is_torch:
            import torch

            return torch.from_numpy(edge[0]), torch.from_numpy(dp[0])
        return edge[0], dp[0]

    __call__ = forward
