"""GPU: the scratch sweep of tests/test_gpu_scratch.py for the 01_train entry points (csrc/cls_head.hip): wsc_cls_loss (a cached
block and a staged table), wsc_roc_thresholds (a cached block), wsc_cls_threshold_counts and wsc_cls_scores_append give the same
bits whatever the scratch held before (fill off, 0x00, 0xFF, 0x3F), and write nothing outside the caller's buffers.

The cases register themselves through the sweep's own `case()` decorator when this module is imported, which is what puts the four
entry points into test_gpu_scratch.CASES -- the table tests/test_scratch_table_host.py holds against include/wsscam.h.  That
module's own parametrisation was fixed when it was imported, so the two cases run here."""
import pytest

from tests import test_gpu_scratch as sweep

pytestmark = pytest.mark.gpu


@sweep.case("cls-loss", "wsc_cls_loss")
def _cls_loss(ctx):
    from tests import cls_head_ref, test_gpu_cls_head as tch

    outs = []
    for kind in ("mean", "max"):
        res = tch.run(ctx, kind, *cls_head_ref.make_case(tch.SMALL[0], kind))
        outs += [res[k] for k in ("loss",) + tch.WANT_ALL]
    return outs


@sweep.case("cls-roc", "wsc_roc_thresholds", "wsc_cls_threshold_counts", "wsc_cls_scores_append")
def _cls_roc(ctx):
    from tests import cls_head_ref
    from wsscam import cls_train
    from wsscam.secdsrg import DeviceMaps

    scores, targets = cls_head_ref.make_scores(400, 20, seed=11)
    with cls_train.ScoreEvaluator(ctx, 20) as ev:
        with DeviceMaps.from_host(ctx, scores[:150]) as first:  # one batch arrives on the device
            ev.update(first, targets[:150])
        ev.update(scores[150:], targets[150:])
        thr, n_points, fps, tps = ev.curve_points()
        return [thr, ev.status, n_points, fps, tps, ev.metrics(thr)["counts"]]


@pytest.mark.parametrize("cid", ["cls-loss", "cls-roc"])
def test_result_does_not_depend_on_scratch(ctx, cid):
    sweep.sweep(ctx, cid)
