"""GPU: the scratch sweep of tests/test_gpu_scratch.py for the update half of a 01_train step (csrc/sgd.hip, csrc/repack.hip, wsc_cls_sgd_step /
wsc_net_cls_load_params of csrc/net.hip): a whole ClsTrainer.step on a VGG16 net -- the arena, cached blocks, the gradient object's
workspace, the repack's partial channel maxima and the transposed copy of the classifier the CAM head is packed from -- gives the same
bits whatever the scratch held before (fill off, 0x00, 0xFF, 0x3F), and writes nothing outside the caller's buffers.

The case registers itself through the sweep's own `case()` decorator when this module is imported, which is what puts the new entry
points -- the layout query included: it runs inside the step's case -- into test_gpu_scratch.CASES, the table
tests/test_scratch_table_host.py holds against include/wsscam.h.  That module's own parametrisation was fixed when it was imported,
so the case runs here."""
import numpy as np
import pytest

from tests import test_gpu_scratch as sweep
from wsscam import _lib

pytestmark = pytest.mark.gpu


@sweep.case("cls-sgd-step", "wsc_cls_param_layout", "wsc_cls_sgd_step", "wsc_net_cls_load_params")
def _sgd_step(ctx):
    from tests import cls_grad_ref as gref
    from tests import cls_sgd_ref as ref
    from wsscam import cls_train
    from wsscam.net import vgg16_cam

    sd = gref.state_dict("vgg16", True)
    m = vgg16_cam.CAM(None, "voc12", "", 20, None, precision=_lib.PREC_F16X3)
    m.load_state_dict(sd)
    m._ctx = ctx
    try:
        with cls_train.ClsTrainer(m, "mean", 20) as tr:
            assert [(e["name"], e["offset"]) for e in tr.grad.param_layout] == [(e[0], e[1]) for e in ref.layout(sd, "vgg16", 20)[0]]
            rng = np.random.default_rng(9)
            metrics = tr.step(gref.net_input((33, 33)), (rng.random((gref.B, 20)) < 0.3).astype(np.float32), 0.01)
            # what the step left in the net: the training forward pass on the repacked rows, the CAM and the score on the refolded
            # BatchNorm and the repacked head
            feat = m.forward_train_dev(gref.net_input((33, 33)), keep=False, bn_keep=None)
            with feat:
                cam, score = m.forward_batch(np.random.default_rng(17).normal(0, 1, (1, 2, 3, 33, 33)).astype(np.float32), want_score=True)
                return [np.array([metrics["loss"]]), tr.params.to_host(), tr.mom.to_host(), tr.grads.to_host(), m.bn_running_dev().to_host(),
                        feat.to_host(), cam, score]
    finally:
        m._release_net()
        m._ctx = None


def test_result_does_not_depend_on_scratch(ctx):
    sweep.sweep(ctx, "cls-sgd-step")
