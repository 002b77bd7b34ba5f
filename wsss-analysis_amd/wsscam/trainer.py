"""What the three trainers (secdsrg.SegTrainer, irn_train.IrnTrainer, cls_train.ClsTrainer) have in common: the resident
buffers and their release, the host view of a buffer through the parameter codec, and the checkpoint file.

A checkpoint is np.save(allow_pickle=True) of ONE dict: the trainer's parameters (`_params_dict`), every slot buffer of SLOTS in
the parameters' shapes under its "__name__" key, the counters under "__step__" (`_step_dict` / `_set_step`), and whatever the
caller adds under further "__name__" keys (save(extra=...), `loaded_extra` after a load)."""
import numpy as np

from . import _lib
from .device import DeviceMaps, Freed


class TrainerCore(Freed):
    """A trainer adds _fields() (the codec table of a buffer), _grad_now() (the gradient object of the net as it is now),
    _params_dict(), _step_dict() and _set_step(step); `grad` is the _lib gradient object it was made with."""
    BUFFERS = ("params", "mom")           # the resident DeviceMaps, `params` first; all of one size and layout
    SLOTS = (("__momentum__", "mom"),)    # (checkpoint key, buffer) of those that travel with a checkpoint beside the parameters
    params = None

    def _init_buffers(self, make_flat, scratch=()):
        """`params` from make_flat(), the other BUFFERS zeros -- those of `scratch` left as allocated; close() on failure"""
        try:
            flat = make_flat()
            for name in self.BUFFERS:
                setattr(self, name, DeviceMaps(self.ctx, flat.shape, np.float32) if name in scratch else
                        DeviceMaps.from_host(self.ctx, flat if name == "params" else np.zeros_like(flat)))
        except Exception:
            self.close()
            raise

    def close(self):
        for name in self.BUFFERS:
            buf = getattr(self, name, None)
            if buf is not None:
                buf.free()
            setattr(self, name, None)

    def free(self):  # (Freed: a context manager closes)
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if self.params is None or self._grad_now() is not self.grad:
            raise ValueError("%s: closed, or the model's net was rebuilt since the trainer was made" % type(self).__name__)

    def _host(self, buf):
        return _lib.unflatten(buf.to_host(), self._fields())

    def params_host(self):
        return self._host(self.params)

    def momentum_host(self):
        return self._host(self.mom)

    def _flat(self, tensors):
        """tensors in the parameters' shapes -> the flat host array of a buffer"""
        return self.grad.flat_params(tensors)

    def _restore_slot(self, name, tensors):
        flat = self._flat(tensors)  # (a slot has the parameters' shapes)
        getattr(self, name).free()
        setattr(self, name, None)
        setattr(self, name, DeviceMaps.from_host(self.ctx, flat))

    def save(self, path, extra=None):
        d = self._params_dict()
        for key, name in self.SLOTS:
            d[key] = self._host(getattr(self, name))
        d["__step__"] = self._step_dict()
        for k, v in (extra or {}).items():
            if not k.startswith("__") or k in d:
                raise ValueError("%s.save: extra key %r (a new name beginning with '__')" % (type(self).__name__, k))
            d[k] = v
        self._write(path, d)

    @staticmethod
    def _write(path, d):
        with open(path, "wb") as fh:  # (np.save appends '.npy' to a bare name, not to a file object)
            np.save(fh, d, allow_pickle=True)

    @staticmethod
    def _read(path):
        """-> (the tensors of the file, its "__name__" entries)"""
        d = np.load(path, encoding="latin1", allow_pickle=True).item()
        return {k: v for k, v in d.items() if not k.startswith("__")}, {k: v for k, v in d.items() if k.startswith("__")}

    def _resume(self, marked):
        """the second half of every load(): the slots, the counters and `loaded_extra` from a file's "__name__" entries into a
        trainer just made from its tensors; close() on failure"""
        try:
            for key, name in self.SLOTS:
                if key in marked:
                    self._restore_slot(name, marked[key])
            self._set_step(marked.get("__step__", {}))
            self.loaded_extra = {k: v for k, v in marked.items() if k != "__step__" and k not in dict(self.SLOTS)}
        except Exception:
            self.close()
            raise
        return self
