"""Arrays that stay on the device between calls, for every training and prediction module.

    DeviceMaps       a C-contiguous array in one pooled device buffer of a context; view() a sub-range of it that owns nothing
    Freed            free() on exit of a `with` block, for the holder classes that wrap one DeviceMaps
    Tape             what a training forward pass keeps for its backward pass: one float32 DeviceMaps and its plan
    device_operand   one operand of a loss class: checked and read in place, or uploaded once
    device_input     the input of a network pass: a live DeviceMaps of the context, read in place, or a host array uploaded once

Nothing here imports the other modules of the package: secdsrg, irn_train, cls_train and net/ all import from here
(secdsrg re-exports DeviceMaps, Freed and device_operand, the path they had before)."""
import numpy as np


class Freed:
    """free() on exit of a `with` block; free() itself releases `maps`, the one DeviceMaps a holder class wraps."""

    def free(self):
        self.maps.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


class DeviceMaps(Freed):
    """A C-contiguous array in ONE pooled device buffer of a context: `shape`, `dtype`, `.ptr` (device address), `.to_host()`,
    `.free()`; a context manager frees it on exit.  The buffer is pooled, so it belongs to its context's stream alone.
    A packed ragged batch of uint8 images (SegNet.preprocess_dev(keep_images=True)) also carries `sizes` [(h, w)] and `offsets`
    (bytes); its shape is the flat byte count."""

    def __init__(self, ctx, shape, dtype=np.float32, buf=None):
        self.ctx = ctx
        self.shape = tuple(int(v) for v in shape)
        self.dtype = np.dtype(dtype)
        self.sizes = self.offsets = None
        self.buf = buf if buf is not None else ctx.alloc(max(self.nbytes, 1), pooled=True)

    @classmethod
    def from_host(cls, ctx, arr, dtype=None):
        """One upload of a host array."""
        a = np.ascontiguousarray(arr, dtype=dtype)
        return cls(ctx, a.shape, a.dtype, ctx.to_device(a, pooled=True))

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    @property
    def ptr(self):
        return None if self.buf is None else self.buf.ptr

    def to_host(self):
        if self.buf is None:
            raise ValueError("DeviceMaps: freed")
        return self.ctx.to_host(self.buf, self.shape, self.dtype)

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None

    def view(self, offset, shape):
        """`shape` elements of this array's dtype from element `offset` on, as a DeviceMaps that owns nothing (DeviceView)."""
        return DeviceView(self, offset, shape)


class DeviceView(DeviceMaps):
    """A range of a DeviceMaps as a DeviceMaps: it owns nothing (free() is a no-op) and dies with its parent."""

    def __init__(self, parent, offset, shape):
        self.ctx, self.shape, self.dtype = parent.ctx, tuple(int(v) for v in shape), parent.dtype
        self.sizes = self.offsets = None
        self._parent, self._at = parent, parent.dtype.itemsize * int(offset)

    @property
    def buf(self):
        return self._parent.buf

    @property
    def ptr(self):
        return None if self._parent.ptr is None else self._parent.ptr + self._at

    def to_host(self):
        if self._parent.buf is None:
            raise ValueError("DeviceMaps: the viewed buffer is freed")
        return self.ctx.to_host(self._parent.buf, self.shape, self.dtype, offset_bytes=self._at)

    def free(self):
        pass


class Tape(Freed):
    """The tape of a training forward pass: `maps` one float32 DeviceMaps of `elems` floats, `entries` the plan the net gave for
    `batch` samples ([{'name', 'Ho', 'Wo', 'C', 'offset'}]).  entry(name) downloads one tensor ([batch][Ho][Wo][C]; a subclass
    says otherwise in entry_shape); free() / a context manager releases the buffer."""

    def __init__(self, maps, entries, batch):
        self.maps, self.entries, self.batch = maps, entries, int(batch)
        self.elems = maps.shape[0]

    def entry_shape(self, e):
        return (self.batch, e["Ho"], e["Wo"], e["C"])

    def entry(self, name):
        e = next(e for e in self.entries if e["name"] == name)
        return self.maps.ctx.to_host(self.maps.buf, self.entry_shape(e), np.float32, offset_bytes=4 * e["offset"])


def device_operand(owner, ctx, name, a, dtype, shape, held):
    """One operand of a loss class as a DeviceMaps of `dtype`: a DeviceMaps is checked and read in place, a host array is uploaded
    once and the upload appended to `held` (the caller frees those).  shape: a tuple to match, a function that says whether the
    shape fits, or None.  A wrong dtype or shape is a ValueError that names the class of `owner` and the argument `name`."""
    who, dtype = type(owner).__name__, np.dtype(dtype)
    on_device = isinstance(a, DeviceMaps)
    if on_device:
        if a.dtype != dtype:
            raise ValueError("%s: %s is %s on the device, not %s" % (who, name, a.dtype, dtype))
    else:
        a = np.asarray(a)
        if a.dtype.kind not in "fiub":
            raise ValueError("%s: %s has dtype %s, not a real number type" % (who, name, a.dtype))
    got = tuple(a.shape)
    if shape is not None and not (shape(got) if callable(shape) else got == tuple(shape)):
        raise ValueError("%s: %s has shape %r%s" % (who, name, got, "" if callable(shape) else ", expected %r" % (tuple(shape),)))
    if on_device:
        return a
    held.append(DeviceMaps.from_host(ctx, a, dtype=dtype))
    return held[-1]


def device_input(ctx, a, dtype, who):
    """"Read in place or upload once": `a` a live DeviceMaps of `dtype` on `ctx`, or a host array / tensor, which is uploaded
    once -> (DeviceMaps, the upload or None).  The caller checks the shape and frees the upload in its `finally`.  Anything else
    on the device is a ValueError that names the caller `who`."""
    if isinstance(a, DeviceMaps):
        if a.dtype != np.dtype(dtype) or a.ctx is not ctx or a.ptr is None:
            raise ValueError("%s: the operand is %s on the device, not a live %s DeviceMaps of this context" % (who, a.dtype, np.dtype(dtype)))
        return a, None
    up = DeviceMaps.from_host(ctx, a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a), dtype=dtype)
    return up, up
