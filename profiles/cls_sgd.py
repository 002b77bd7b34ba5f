"""One 01_train step on the device split into its parts, next to the host rebuild the device update replaces.

  net          argv[1]: vgg16 | m7 (default vgg16), VOC2012 (20 classes), BatchNorm, real widths, MaxPool2d(2, 2);
               B (argv[2], default 8) images of S x S (argv[3], default 321), f16x3 forward
  parts        wsc_net_forward_cls_train, wsc_cls_loss (reading the Linear from the parameter buffer's tail, writing its gradient
               into the gradient buffer's tail), wsc_net_backward_cls, wsc_cls_sgd_step, wsc_net_cls_load_params -- the five calls
               of cls_train.ClsTrainer.step, each on its own with wsc_timer_* on the ctx stream; then ClsTrainer.step itself, wall
               clock with a synchronisation (the download of the six loss values ends it anyway)
  rebuild      what a trainer without the device update does after updating on the host: download the gradients (ClsGrads.
               to_state_dict), build a new net from the state dict (_lib.Net: host packing of every layer, the BatchNorm fold,
               two uploads) and a new ClsGrad (the rotated data-gradient kernels); wall clock

Prints one JSON line: ms per call, [median, min, max] over RUNS windows of REPS calls.
One GPU step per invocation; run it under its own time limit:   timeout -k 10 600 python profiles/cls_sgd.py [net] [B] [S]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from oracle import cnn_ref  # noqa: E402
from wsscam import _lib, cls_train  # noqa: E402
from wsscam.net import m7_cam, vgg16_cam  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

NET = sys.argv[1] if len(sys.argv) > 1 else "vgg16"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
S = int(sys.argv[3]) if len(sys.argv) > 3 else 321
WARM, RUNS = 2, 5
C = 20

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


def wall(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)]


cls, cfg, pool = (vgg16_cam.CAM, cnn_ref.VGG16_CFG, "mean") if NET == "vgg16" else (m7_cam.CAM, cnn_ref.M7_CFG, "max")
model = cls(None, "voc12", "", C, None, precision=_lib.PREC_F16X3)
model.load_state_dict(cnn_ref.make_plain_state_dict(NET, cfg, C, True, seed=1))
model._ctx = ctx
x = DeviceMaps.from_host(ctx, rng.standard_normal((B, 3, S, S)).astype(np.float32))
targets_host = (rng.random((B, C)) < 0.3).astype(np.float32)
targets = DeviceMaps.from_host(ctx, targets_host)
net = model._ensure_net()
F = net.feat_channels()
with cls_train.ClsTrainer(model, pool, C) as tr:
    grad = tr.grad
    entries, elems = net.cls_tape_plan(B, S, S)
    h, wd = net.cam_size_hw(S, S)
    feat, tape = DeviceMaps(ctx, (B, h, wd, F)), DeviceMaps(ctx, (elems,))
    g_feat, loss_dev = DeviceMaps(ctx, (B, h, wd, F)), DeviceMaps(ctx, (6,), np.float64)
    run = model.bn_running_dev()
    (w, bias), (g_w, g_b) = tr._tail_views(tr.params), tr._tail_views(tr.grads)
    out = {"net": NET, "B": B, "S": S, "precision": "f16x3", "tape_MB": round(elems * 4 / 1e6, 1), "parameters": grad.param_elems,
           "forward_train_ms": timed(lambda: net.forward_cls_train(x.ptr, B, S, S, tape.ptr, elems, feat.ptr, run_dev=run.ptr), 3),
           "cls_loss_ms": timed(lambda: _lib.cls_loss(ctx, feat.ptr, B, h * wd, F, tr.loss.pool, w.ptr, bias.ptr, C, targets.ptr, None, loss_dev.ptr,
                                                      grad_feat_dev=g_feat.ptr, grad_w_dev=g_w.ptr, grad_bias_dev=g_b.ptr), 3),
           "backward_ms": timed(lambda: grad.backward(B, S, S, tape.ptr, elems, g_feat.ptr, tr.grads.ptr), 3),
           # (lr = 0: the timed loop must not walk the parameters away; the kernel does the same work)
           "sgd_step_ms": timed(lambda: grad.sgd_step(tr.params.ptr, tr.grads.ptr, tr.mom.ptr, 0.0, 0.9, True), 20),
           "load_params_ms": timed(lambda: grad.load_params(tr.params.ptr, run.ptr), 20)}
    for m in (feat, tape, g_feat, loss_dev):
        m.free()
    out["trainer_step_wall_ms"] = wall(lambda: tr.step(x, targets, 0.0), 5)

    def rebuild():
        grads = cls_train.ClsGrads(tr.grads, grad.layout).to_state_dict()  # the download a host update needs
        sd = model._extra_tensors(model._sd)
        n2 = _lib.Net(ctx, model.arch, sd, C, _lib.PREC_F16X3)
        g2 = _lib.ClsGrad(n2, sd)
        g2.close()
        n2.close()
        return grads

    out["host_rebuild_wall_ms"] = wall(rebuild, 3)
ctx.sync()
print(json.dumps(out))
