"""GPU: the scratch sweep of tests/test_gpu_scratch.py for the 01_train batch stage (csrc/cls_batch.hip, wsc_cls_train_batch): a ragged
B = 3 batch with the warp -- its job records and PIL's nearest-index tables travel in the staged table, the call's only scratch --
gives the same bits whatever the scratch held before (fill off, 0x00, 0xFF, 0x3F), and writes nothing outside the caller's buffers.

The case registers itself through the sweep's own `case()` decorator when this module is imported, which is what puts the new entry
point into test_gpu_scratch.CASES, the table tests/test_scratch_table_host.py holds against include/wsscam.h.  That module's own
parametrisation was fixed when it was imported, so the case runs here."""
import numpy as np
import pytest

from tests import test_gpu_scratch as sweep
from wsscam import _lib

pytestmark = pytest.mark.gpu


@sweep.case("cls-train-batch", "wsc_cls_train_batch")
def _cls_train_batch(ctx):
    from tests import cls_batch_ref as ref

    hw = (17, 33)
    images = [ref.image(51, (40, 31)), ref.image(52, (5, 23)), ref.image(53, hw)]
    affine, flags = ref.voc_draws(6, hw[0], hw[1], 3)
    flags[2] |= ref.FLAG_FLIP_ROWS
    offs = np.concatenate([[0], np.cumsum([i.size for i in images])]).astype(np.int64)
    src = ctx.to_device(np.concatenate([i.reshape(-1) for i in images]))
    outs = []
    for mode, name in (("reflect", "VOC2012"), ("constant", "ADP")):
        x = sweep.out(ctx, (3, 3) + hw)
        _lib.cls_train_batch(ctx, src, [i.shape[:2] for i in images], offs[:-1], hw, affine, flags, mode, 37.5, *ref.STANDARDISE[name], x)
        got = sweep.host(ctx, x, (3, 3) + hw)
        assert np.array_equal(got.view(np.uint32), ref.batch(images, hw, affine, flags, mode, 37.5, *ref.STANDARDISE[name]).view(np.uint32))
        outs.append(got)
    return outs


def test_result_does_not_depend_on_scratch(ctx):
    sweep.sweep(ctx, "cls-train-batch")
