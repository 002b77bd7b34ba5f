"""wsc_cls_loss and wsc_roc_thresholds at the reference's sizes, timed with wsc_timer_* on the ctx stream.

  cls_loss   B = 16 (argv[1]), n = 41 x 41, F = 1024, C = 20, mean pool (argv[2]: mean | max): the call with no gradient (pool +
             dense + finish launches), with grad_w / grad_bias, with grad_feat, and with all of them -- the differences are the
             wgrad and feat_grad launches.  The map is 110 MB at B = 16: read once by the pool kernel (once more by the max pool's
             feat_grad kernel), written once as grad_feat.
  roc        N = 1449, C = 20: wsc_roc_thresholds with the curve outputs, wsc_cls_threshold_counts

Prints one JSON line: ms per call, [median, min, max] over RUNS windows of REPS calls.
One GPU step per invocation; run it under its own time limit:   timeout -k 10 300 python profiles/cls_head.py [B] [pool]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import cls_head_ref as ref  # noqa: E402
from wsscam import _lib  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
KIND = sys.argv[2] if len(sys.argv) > 2 else "mean"
n, F, C = 41 * 41, 1024, 20
WARM, REPS, RUNS = 3, 200, 5

ctx = _lib.Context(0)
rng = np.random.default_rng(3)
feat = DeviceMaps.from_host(ctx, rng.normal(0, 1, (B, n, F)).astype(np.float32))
w = DeviceMaps.from_host(ctx, (rng.normal(0, 1, (C, F)) * 2).astype(np.float32))
target = DeviceMaps.from_host(ctx, (rng.random((B, C)) < 0.4).astype(np.float32))
loss = DeviceMaps(ctx, (len(_lib.CLS_LOSS_SLOTS),), np.float64)
g_feat, g_w, g_bias = DeviceMaps(ctx, (B, n, F)), DeviceMaps(ctx, (C, F)), DeviceMaps(ctx, (C,))
pool = {"mean": _lib.CLS_POOL_MEAN, "max": _lib.CLS_POOL_MAX}[KIND]


def timed(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(RUNS):
        ctx.timer_begin()
        for _ in range(REPS):
            fn()
        ms.append(ctx.timer_end() / REPS)
    return [round(float(np.median(ms)), 4), round(min(ms), 4), round(max(ms), 4)]


def cls(feat_grad, w_grad):
    return lambda: _lib.cls_loss(ctx, feat.ptr, B, n, F, pool, w.ptr, None, C, target.ptr, None, loss.ptr,
                                 grad_feat_dev=g_feat.ptr if feat_grad else None, grad_w_dev=g_w.ptr if w_grad else None,
                                 grad_bias_dev=g_bias.ptr if w_grad else None)


out = {"B": B, "pool": KIND, "map_MB": round(B * n * F * 4 / 1e6, 1),
       "cls_loss_ms": {"loss_only": timed(cls(False, False)), "with_grad_w": timed(cls(False, True)),
                       "with_grad_feat": timed(cls(True, False)), "all": timed(cls(True, True))}}

N = 1449
scores_h, targets_h = ref.make_scores(N, C, seed=11)
scores, targets = DeviceMaps.from_host(ctx, scores_h), DeviceMaps.from_host(ctx, targets_h)
thr, status, n_points = DeviceMaps(ctx, (C,)), DeviceMaps(ctx, (C,), np.int32), DeviceMaps(ctx, (C,), np.int32)
fps, tps, counts = DeviceMaps(ctx, (C, N + 1), np.int32), DeviceMaps(ctx, (C, N + 1), np.int32), DeviceMaps(ctx, (C, 5), np.int64)
out["roc_ms"] = {"N": N, "C": C,
                 "roc_thresholds": timed(lambda: _lib.roc_thresholds(ctx, scores.ptr, targets.ptr, N, C, thr.ptr, status.ptr, n_points.ptr,
                                                                     fps.ptr, tps.ptr)),
                 "threshold_counts": timed(lambda: _lib.cls_threshold_counts(ctx, scores.ptr, targets.ptr, N, C, thr.ptr, counts.ptr))}
print(json.dumps(out))
