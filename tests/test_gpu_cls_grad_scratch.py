"""GPU: the scratch sweep of tests/test_gpu_scratch.py for the training pass of the plain stacks (csrc/cls_grad.hip, the pool gradients
of csrc/pool.hip, wsc_net_forward_cls_train / wsc_net_backward_cls of csrc/net.hip): the BatchNorm kernels (a cached block: tickets,
partials), the pool gradients, and a whole step on an M7 net (the arena, cached blocks, the gradient object's own workspace) give the
same bits whatever the scratch held before (fill off, 0x00, 0xFF, 0x3F), and write nothing outside the caller's buffers.

The cases register themselves through the sweep's own `case()` decorator when this module is imported, which is what puts the new
entry points -- the plan / layout queries and the destroy included: they run inside the step's case -- into test_gpu_scratch.CASES,
the table tests/test_scratch_table_host.py holds against include/wsscam.h.  That module's own parametrisation was fixed when it was
imported, so the cases run here."""
import numpy as np
import pytest

from tests import test_gpu_scratch as sweep
from wsscam import _lib

pytestmark = pytest.mark.gpu


@sweep.case("cls-batch-norm", "wsc_batch_norm_train_nhwc", "wsc_batch_norm_grad_nhwc")
def _batch_norm(ctx):
    from tests import test_gpu_cls_grad as tcg

    outs = []
    for M, C in ((297, 64), (30, 1024)):
        a, gamma, beta, dy, run0 = tcg.bn_case(M, C)
        stats, y, run = tcg.run_bn_train(ctx, a, gamma, beta, run0)
        outs += [stats, y, run] + list(tcg.run_bn_grad(ctx, a, stats, gamma, dy))
    return outs


@sweep.case("cls-pool-grad", "wsc_pool_tf_grad_nhwc", "wsc_maxpool_grad_nhwc")
def _pool_grad(ctx):
    from tests import test_gpu_cls_grad as tcg

    return [tcg.run_pool_grad(ctx, *tcg.pool_case(pool, (7, 9), "relu")[:2], pool) for pool in (("tf", 3, 2, 1), ("tf", 2, 1, 0), ("torch", 2, 2, 0))]


@sweep.case("cls-train-step", "wsc_net_cls_tape_plan", "wsc_net_forward_cls_train", "wsc_cls_grad_create", "wsc_cls_grad_layout",
            "wsc_net_backward_cls", "wsc_cls_grad_destroy")
def _train_step(ctx):
    from tests import cls_grad_ref as gref
    from wsscam.net import m7_cam
    from wsscam.secdsrg import DeviceMaps

    case = ("m7", True, gref.KERAS_POOLS, (33, 33))
    m = m7_cam.CAM(None, "voc12", "", 20, None, precision=_lib.PREC_F16X3, pooling=gref.KERAS_POOLS)
    m.load_state_dict(gref.state_dict("m7", True))
    m._ctx = ctx
    try:
        feat, tape = m.forward_train_dev(gref.net_input(case[3]))
        with feat, tape, DeviceMaps.from_host(ctx, gref.case_dfeat(case, feat.shape)) as dfeat, m.backward_dev(tape, dfeat) as grads:
            assert [e["name"] for e in grads.layout] == gref.param_names("m7", gref.state_dict("m7", True))
            # (entry by entry: the floats between the tape's entries are not written)
            return [feat.to_host(), grads.maps.to_host(), m.bn_running_dev().to_host()] + [tape.entry(e["name"]) for e in tape.entries]
    finally:
        m._release_net()
        m._ctx = None


@pytest.mark.parametrize("cid", ["cls-batch-norm", "cls-pool-grad", "cls-train-step"])
def test_result_does_not_depend_on_scratch(ctx, cid):
    sweep.sweep(ctx, cid)
