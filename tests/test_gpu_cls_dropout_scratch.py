"""GPU: the scratch sweep of tests/test_gpu_scratch.py for the dropout sites of the 01_train training step (csrc/cls_grad.hip's
BatchNorm apply with dropout and BatchNorm gradient with a regenerated mask; wsc_net_forward_cls_train_drop /
wsc_net_backward_cls_drop of csrc/net.hip): the dropped forward / backward results do not depend on what the workspace arena, the
cached blocks, the gradient object's workspace -- the pooled buffers of M7's site among them -- held before (fill off, 0x00, 0xFF,
0x3F), and nothing is written outside the caller's buffers.

The cases register themselves through the sweep's own `case()` decorator when this module is imported, which is what puts the new
entry points -- wsc_net_cls_feat_dims included: it runs inside the step's case -- into test_gpu_scratch.CASES, the table
tests/test_scratch_table_host.py holds against include/wsscam.h.  That module's own parametrisation was fixed when it was imported,
so the cases run here."""
import pytest

from tests import test_gpu_scratch as sweep
from wsscam import _lib

pytestmark = pytest.mark.gpu


@sweep.case("cls-drop-batch-norm", "wsc_batch_norm_train_drop_nhwc", "wsc_batch_norm_grad_drop_nhwc")
def _batch_norm_drop(ctx):
    from tests import test_gpu_cls_dropout as tcd
    from tests import test_gpu_cls_grad as tcg

    outs = []
    for (M, C), p in (((297, 64), 0.5), ((30, 1024), 0.3)):
        a, gamma, beta, dy, run0 = tcg.bn_case(M, C)
        stats, y, run = tcd.run_bn_train_drop(ctx, a, gamma, beta, run0, p)
        outs += [stats, y, run] + list(tcd.run_bn_grad_drop(ctx, a, stats, gamma, dy, p))
    return outs


def _step(ctx, root, bn, pools, hw, prec):
    from tests import cls_dropout_ref as dref
    from tests import cls_grad_ref as gref
    from wsscam.net import m7_cam, vgg16_cam
    from wsscam.secdsrg import DeviceMaps

    case = (root, bn, pools, hw)
    m = (vgg16_cam.CAM if root == "vgg16" else m7_cam.CAM)(None, "voc12", "", 20, None, precision=prec, pooling=pools)
    m.load_state_dict(gref.state_dict(root, bn))
    m._ctx = ctx
    try:
        feat, tape = m.forward_train_dev(gref.net_input(hw), dropout=dref.DROP)
        assert tuple(feat.shape[1:3]) == m._ensure_net().cls_feat_dims(hw[0], hw[1], True)
        with feat, tape, DeviceMaps.from_host(ctx, gref.case_dfeat(case, feat.shape)) as dfeat, m.backward_dev(tape, dfeat) as grads:
            # (entry by entry: the floats between the tape's entries are not written)
            return [feat.to_host(), grads.maps.to_host(), m.bn_running_dev().to_host()] + [tape.entry(e["name"]) for e in tape.entries]
    finally:
        m._release_net()
        m._ctx = None


@sweep.case("cls-drop-train-step-m7", "wsc_net_cls_feat_dims", "wsc_net_forward_cls_train_drop", "wsc_net_backward_cls_drop")
def _train_step_m7(ctx):
    from tests import cls_grad_ref as gref

    return _step(ctx, "m7", True, gref.KERAS_POOLS, (33, 33), _lib.PREC_F16X3)


@sweep.case("cls-drop-train-step-vgg16", "wsc_net_forward_cls_train_drop", "wsc_net_backward_cls_drop")
def _train_step_vgg16(ctx):
    return _step(ctx, "vgg16", True, None, (33, 33), _lib.PREC_F16X3)


@pytest.mark.parametrize("cid", ["cls-drop-batch-norm", "cls-drop-train-step-m7", "cls-drop-train-step-vgg16"])
def test_result_does_not_depend_on_scratch(ctx, cid):
    sweep.sweep(ctx, cid)
