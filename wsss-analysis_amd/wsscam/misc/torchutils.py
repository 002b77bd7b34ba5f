"""misc.torchutils helpers of the CAM path (upstream jiwoon-ahn/irn semantics, SURVEY.md
Appendix A; call site: 03b_irn/step/make_cam.py:120) and PolyOptimizer, the optimiser of
step/train_irn.py:86-90, on the device."""
import numpy as np


class Subset:
    """torch.utils.data.Subset without the torch dependency."""

    def __init__(self, dataset, indices):
        self.dataset = dataset
        self.indices = indices

    def __getitem__(self, idx):
        return self.dataset[int(self.indices[idx])]

    def __len__(self):
        return len(self.indices)


def split_dataset(dataset, n_splits):
    """Round-robin shards: GPU g of G owns images[g::G]."""
    return [Subset(dataset, np.arange(i, len(dataset), n_splits)) for i in range(n_splits)]


def gap2d(x, keepdims=False):
    out = x.reshape(x.shape[0], x.shape[1], -1).mean(-1)
    if keepdims:
        out = out.reshape(out.shape[0], out.shape[1], 1, 1)
    return out


class PolyOptimizer:
    """misc.torchutils.PolyOptimizer as step/train_irn.py:86-90, 127-129 uses it, on the device: torch.optim.SGD (dampening 0,
    no Nesterov) over two parameter groups with a poly schedule.

        PolyOptimizer(groups, lr, weight_decay, max_step, momentum=0.9, sgd_momentum=None)
          groups        the _lib.IrnGrad of the net: its layout is trainable_parameters() -- param_groups[0] the `fc_edge*`
                        entries at lr, param_groups[1] the rest at 10 lr (train_irn.py:87-88), both at weight_decay
          momentum      the POLY EXPONENT (upstream's name for it): before each step, while global_step < max_step, a group's
                        rate is lr0_group * (1 - global_step / max_step) ** momentum; from max_step on it keeps its last value
          sgd_momentum  the momentum of the SGD step.  None: the value of weight_decay.  Upstream's constructor calls
                        super().__init__(params, lr, weight_decay), and the third positional argument of torch.optim.SGD is
                        `momentum`: the SGD momentum IS the weight-decay value there, and 0.9 only the exponent (a subclass
                        written that way reports param_groups[0]['momentum'] == weight_decay; the upstream file itself is not
                        part of the reference tree, so this is the behaviour as reconstructed from its call site and
                        SURVEY.md).  Pass 0.9 for conventional momentum.
        lr_now()        the two rates of the next step, Python doubles
        step(params, grads, mom)   one update of three float32 DeviceMaps of groups.grad_elems floats (wsc_irn_sgd_step: the
                        rates cross as float, the cast torch applies for fp32 tensors), then global_step += 1; grads is only read
    """

    def __init__(self, groups, lr, weight_decay, max_step, momentum=0.9, sgd_momentum=None):
        if int(max_step) < 1:
            raise ValueError("PolyOptimizer: max_step = %r" % (max_step,))
        self.groups = groups
        self.initial_lr = (float(lr), 10 * float(lr))
        self.weight_decay = float(weight_decay)
        self.max_step = int(max_step)
        self.momentum = float(momentum)
        self.sgd_momentum = self.weight_decay if sgd_momentum is None else float(sgd_momentum)
        self.global_step = 0

    def lr_now(self):
        t = min(self.global_step, self.max_step - 1)  # (from max_step on: the last value the schedule set)
        mult = (1 - t / self.max_step) ** self.momentum
        return tuple(lr0 * mult for lr0 in self.initial_lr)

    def step(self, params, grads, mom):
        n = self.groups.grad_elems
        for name, m in (("params", params), ("grads", grads), ("mom", mom)):
            if getattr(m, "ptr", None) is None or np.dtype(m.dtype) != np.float32 or tuple(m.shape) != (n,) or m.ctx is not self.groups.ctx:
                raise ValueError("PolyOptimizer.step: %s is no live float32 DeviceMaps of (%d,) on the net's context" % (name, n))
        lr_edge, lr_dp = self.lr_now()
        self.groups.sgd_step(params.ptr, grads.ptr, mom.ptr, lr_edge, lr_dp, self.weight_decay, self.sgd_momentum)
        self.global_step += 1
