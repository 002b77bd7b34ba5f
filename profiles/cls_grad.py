"""The training pass of the plain stacks at the reference's sizes, timed with wsc_timer_* on the ctx stream.

  batch_norm   per VGG16 layer width at B (argv[1], default 16) images of S x S (argv[2], default 224): wsc_batch_norm_train_nhwc
               (statistics + output: a read twice, y written once) and wsc_batch_norm_grad_nhwc (a and dy read twice, da written
               once) on the layer's [M][C] map, with the bytes each moves and the rate that makes
  step         VGG16 with BatchNorm (argv[3]: f16x3 | f32), MaxPool2d(2, 2): wsc_net_forward_cls_train into a tape, wsc_cls_loss
               with all its gradients, wsc_net_backward_cls -- the three parts of cls_train.grad_step, each on its own

Prints one JSON line: ms per call, [median, min, max] over RUNS windows of REPS calls.
One GPU step per invocation; run it under its own time limit:   timeout -k 10 600 python profiles/cls_grad.py [B] [S] [precision]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from oracle import cnn_ref  # noqa: E402
from wsscam import _lib, cls_train  # noqa: E402
from wsscam.net import vgg16_cam  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
S = int(sys.argv[2]) if len(sys.argv) > 2 else 224
PREC = {"f16x3": _lib.PREC_F16X3, "f32": _lib.PREC_F32}[sys.argv[3] if len(sys.argv) > 3 else "f16x3"]
WARM, RUNS = 2, 5

ctx = _lib.Context(0)
rng = np.random.default_rng(3)


def timed(fn, reps):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(RUNS):
        ctx.timer_begin()
        for _ in range(reps):
            fn()
        ms.append(ctx.timer_end() / reps)
    return [round(float(np.median(ms)), 4), round(min(ms), 4), round(max(ms), 4)]


out = {"B": B, "S": S, "precision": sys.argv[3] if len(sys.argv) > 3 else "f16x3", "batch_norm": []}
for C, div in ((64, 1), (128, 2), (256, 4), (512, 8), (1024, 8)):  # the map of VGG16's layer1 .. layer5
    M = B * (S // div) ** 2
    a = DeviceMaps.from_host(ctx, rng.standard_normal((M, C)).astype(np.float32))
    dy, y, da = DeviceMaps.from_host(ctx, rng.standard_normal((M, C)).astype(np.float32)), DeviceMaps(ctx, (M, C)), DeviceMaps(ctx, (M, C))
    gamma, beta = DeviceMaps.from_host(ctx, np.ones(C, np.float32)), DeviceMaps.from_host(ctx, np.zeros(C, np.float32))
    stats, dg, db, run = DeviceMaps(ctx, (C, 2)), DeviceMaps(ctx, (C,)), DeviceMaps(ctx, (C,)), DeviceMaps.from_host(ctx, np.ones((2, C), np.float32))
    fwd = timed(lambda: _lib.batch_norm_train_nhwc(ctx, a.ptr, M, C, gamma.ptr, beta.ptr, 1e-3, 0.99, True, run.ptr, stats.ptr, y.ptr), 20)
    bwd = timed(lambda: _lib.batch_norm_grad_nhwc(ctx, a.ptr, stats.ptr, gamma.ptr, dy.ptr, M, C, da.ptr, dg.ptr, db.ptr), 20)
    mb = M * C * 4 / 1e6
    out["batch_norm"].append({"M": M, "C": C, "map_MB": round(mb, 1), "train_ms": fwd, "train_GBps": round(3 * mb / fwd[0], 1),
                              "grad_ms": bwd, "grad_GBps": round(5 * mb / bwd[0], 1)})
    for m in (a, dy, y, da, gamma, beta, stats, dg, db, run):
        m.free()

model = vgg16_cam.CAM(None, "voc12", "", 20, None, precision=PREC)
model.load_state_dict(cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, 20, True, seed=1))
model._ctx = ctx
loss = cls_train.ClsLoss(ctx, "mean", 20)
x = DeviceMaps.from_host(ctx, rng.standard_normal((B, 3, S, S)).astype(np.float32))
targets = DeviceMaps.from_host(ctx, (rng.random((B, 20)) < 0.3).astype(np.float32))
w, bias = [DeviceMaps.from_host(ctx, v) for v in model.classifier_params()]
net = model._ensure_net()
entries, elems = net.cls_tape_plan(B, S, S)
h, wd = net.cam_size_hw(S, S)
feat, tape = DeviceMaps(ctx, (B, h, wd, 1024)), DeviceMaps(ctx, (elems,))
run, grad = model.bn_running_dev(), model.cls_grad()
g_feat, g_w, g_b, loss_dev = DeviceMaps(ctx, (B, h, wd, 1024)), DeviceMaps(ctx, (20, 1024)), DeviceMaps(ctx, (20,)), DeviceMaps(ctx, (6,), np.float64)
g_all = DeviceMaps(ctx, (grad.grad_elems,))
out["step"] = {
    "tape_MB": round(elems * 4 / 1e6, 1), "parameters": grad.grad_elems,
    "forward_train_ms": timed(lambda: net.forward_cls_train(x.ptr, B, S, S, tape.ptr, elems, feat.ptr, run_dev=run.ptr), 3),
    "cls_loss_ms": timed(lambda: _lib.cls_loss(ctx, feat.ptr, B, h * wd, 1024, _lib.CLS_POOL_MEAN, w.ptr, bias.ptr, 20, targets.ptr, None, loss_dev.ptr,
                                               grad_feat_dev=g_feat.ptr, grad_w_dev=g_w.ptr, grad_bias_dev=g_b.ptr), 3),
    "backward_ms": timed(lambda: grad.backward(B, S, S, tape.ptr, elems, g_feat.ptr, g_all.ptr), 3)}
ctx.sync()
print(json.dumps(out))
