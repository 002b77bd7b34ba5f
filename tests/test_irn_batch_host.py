"""CPU: the bindings of the IRNet batch entry points (wsscam._lib.pil_resize_u8 / irn_train_batch) reject bad shapes and dtypes
before any C call, and step.train_irn.run refuses an unknown dataset with the reference's KeyError."""
import types

import numpy as np
import pytest

from wsscam import _lib


class _NoCalls:
    """stands in for a context: any use of the library is a failure"""

    h = None

    @property
    def _lib(self):
        raise AssertionError("the binding reached the C library")


def test_symbols_declared_and_bound(built):
    declared = _lib.check_exports()
    assert "wsc_pil_resize_u8" in declared and "wsc_irn_train_batch" in declared
    assert _lib.IRN_BATCH_PARAMS == ("scaled_h", "scaled_w", "flip", "cont_top", "cont_left", "img_top", "img_left", "ch", "cw")
    assert [_lib.irn_reduced_size(S) for S in (32, 34, 30, 512, 2)] == [8, 8, 8, 128, 0]


GOOD_RESIZE = dict(sizes=[(5, 7), (9, 4)], offsets=np.array([0, 105]), out_sizes=[(3, 3), (4, 4)], out_offsets=np.array([0, 27]), channels=3, order=3)


@pytest.mark.parametrize("change", [
    dict(sizes=[(5, 7)]),                                   # one size for two images
    dict(sizes=[(5.5, 7), (9, 4)]),                         # no whole numbers
    dict(sizes=[(0, 7), (9, 4)]),                           # an empty image
    dict(out_sizes=[(3, 3), (4, 40000)]),                   # a side beyond 32768
    dict(out_sizes=[(3, 3, 3), (4, 4, 3)]),
    dict(offsets=np.array([0.0, 105.0])),                   # float offsets
    dict(offsets=np.array([0, -1])),
    dict(out_offsets=np.array([0, 27, 54])),
    dict(channels=2), dict(channels=4),
    dict(sizes=[]),                                         # B = 0
])
def test_pil_resize_binding_rejects(change):
    kw = dict(GOOD_RESIZE, **change)
    with pytest.raises(ValueError):
        _lib.pil_resize_u8(_NoCalls(), 4096, kw["sizes"], kw["offsets"], kw["out_sizes"], kw["out_offsets"], kw["channels"], kw["order"], 8192)


GOOD_BATCH = dict(sizes=[(20, 25), (50, 60)], image_offsets=np.array([0, 1500]), label_offsets=np.array([0, 500]),
                  params=np.array([(24, 30, 0, 5, 2, 0, 0, 24, 30), (45, 54, 1, 0, 0, 9, 17, 32, 32)], np.int32), S=32,
                  mean=(104.0, 117.0, 123.0), std=(255.0, 255.0, 255.0))


@pytest.mark.parametrize("change", [
    dict(params=np.zeros((2, 8), np.int32)),                # a record of eight
    dict(params=np.zeros((3, 9), np.int32)),                # three records for two samples
    dict(params=np.zeros((2, 9), np.float32)),              # float records
    dict(sizes=[(20, 25)]),
    dict(sizes=[(20, 25), (50, 0)]),
    dict(image_offsets=np.array([0])),
    dict(label_offsets=np.array([0.5, 1.0])),
    dict(label_offsets=np.array([-4, 0])),
    dict(mean=(104.0, 117.0)),
    dict(std=(255.0, 0.0, 255.0)),
    dict(std=(255.0, float("nan"), 255.0)),
    dict(S=1), dict(S=32.5), dict(S=10000),
])
def test_train_batch_binding_rejects(change):
    kw = dict(GOOD_BATCH, **change)
    with pytest.raises(ValueError):
        _lib.irn_train_batch(_NoCalls(), 4096, 8192, kw["sizes"], kw["image_offsets"], kw["label_offsets"], kw["params"], kw["S"], kw["mean"],
                             kw["std"], False, 1, 12288, 16384, 20480)


def test_run_refuses_an_unknown_dataset():
    from wsscam.step import train_irn

    args = types.SimpleNamespace(dataset="cityscapes", irn_crop_size=64, irn_batch_size=2, train_list="t", infer_list="i", ir_label_out_dir="l",
                                 dev_root="r", crop_method="random", rescale_range=(0.5, 1.5), outsize=None, norm_mode="int")
    with pytest.raises(KeyError) as ei:
        train_irn.run(args)
    assert ei.value.args[0] == "Dataset cityscapes not yet implemented"


def test_batcher_rejects_before_the_device():
    from wsscam import irn_train

    with pytest.raises(ValueError):
        irn_train.TrainBatcher(_NoCalls(), 64, "int", outsize=(64, 64), rescale=(0.5, 1.5))
    with pytest.raises(ValueError):
        irn_train.TrainBatcher(_NoCalls(), 64, "bytes")
    b = irn_train.TrainBatcher(_NoCalls(), 32, "int")
    img, lab = np.zeros((20, 25, 3), np.uint8), np.zeros((20, 25), np.uint8)
    rec = np.array([(20, 25, 0, 0, 0, 0, 0, 20, 25)], np.int32)
    for images, labels, params in (([img.astype(np.float32)], [lab], rec), ([img], [lab[:10]], rec), ([img], [lab, lab], rec),
                                   ([img], [lab], rec[:, :8]), ([img[..., 0]], [lab], rec), ([], [], rec[:0])):
        with pytest.raises(ValueError):
            b.apply(images, labels, params)
    with pytest.raises(ValueError):  # a record that resizes to another size than outsize
        irn_train.TrainBatcher(_NoCalls(), 32, "int", outsize=(32, 32)).apply([img], [lab], rec)
