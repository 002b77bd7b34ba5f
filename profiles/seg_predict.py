"""One Model.predict batch (03a_sec-dsrg model.py:542-586 with eval_miou) two ways, and rescale_output two ways, at the reference's
size: 321 x 321 network input, 41 x 41 maps, 21 classes, batch 16 (an assumption: the reference takes its batch size from the
command line), DSRG, f16x3, He-scaled random weights at the real widths; 16 synthetic RGB images of 375 x 500 with ground truths
of that size, the VOC test CRF configuration (SEC.py:20: 10 iterations).

    host      SegNet.preprocess + SegNet.softmax + SegEvaluator.update on host arrays: the chain with numpy between the stages
              (code this tree does not change, so it is the parent commit's path)
    device    secdsrg.Predictor.update: the same stages with the maps left on the device
    rescale_host   SegNet.rescale_output     (six more host copies, the (B, 321, 321, C) floats downloaded)
    rescale_dev    SegNet.rescale_output_dev (the result stays on the device; the step synchronises before the clock stops)
Wall-clock time per batch around a synchronised call: WARM warm-up batches, then REPS repeats, median and (min, max).  Prints one
JSON line per step.

Every step is a GPU step of its own; run each under its own time limit, chained so that a failing one stops the rest:
    timeout -k 10 240 python profiles/seg_predict.py host && timeout -k 10 240 python profiles/seg_predict.py device && \
    timeout -k 10 240 python profiles/seg_predict.py rescale_host && timeout -k 10 240 python profiles/seg_predict.py rescale_dev"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import deeplab_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402

B, S, C, REPS, WARM = 16, 321, 21, 5, 2
GT_HW = (375, 500)
WIDTHS = (64, 128, 256, 512, 512)
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 10}
STEPS = ("host", "device", "rescale_host", "rescale_dev")


def inputs():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:GT_HW[0], 0:GT_HW[1]]
    imgs, gts = [], []
    for b in range(B):  # smooth colour fields with noise, blobs of classes: what a CRF has edges to work with
        base = np.stack([127 + 100 * np.sin(yy / (20.0 + 3 * b) + c) * np.cos(xx / (31.0 + 2 * c)) for c in range(3)], -1)
        imgs.append(np.clip(base + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8))
        gts.append(((yy // 47 + xx // 61 + b) % C).astype(np.uint8))
    return imgs, gts


def spread(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2)}


def timed(ctx, call):
    ts = []
    for i in range(WARM + REPS):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        if i >= WARM:
            ts.append(time.perf_counter() - t0)
    return spread(ts)


def main(step):
    ctx = _lib.Context(0)
    weights = ref.random_weights("DSRG", C, fc_width=1024, seed=21, widths=WIDTHS)
    imgs, gts = inputs()
    out = {"step": step, "batch": B, "input": [S, S], "classes": C, "precision": "f16x3", "reps": REPS, "warmup": WARM}
    if step in ("host", "rescale_host", "rescale_dev"):
        net = secdsrg.SegNet("DSRG", weights, C, precision=_lib.PREC_F16X3, ctx=ctx)
        if step == "host":
            ev = secdsrg.SegEvaluator(C, CFG, ctx=ctx)

            def call():
                x = net.preprocess(imgs, MEAN, size=(S, S))
                ev.update(list(net.softmax(x)), imgs, gts)

            out.update(timed(ctx, call))
            out["mIoU"] = ev.metrics()["mIoU"]
            ev.close()
        else:
            x = net.preprocess(imgs, MEAN, size=(S, S))
            if step == "rescale_host":
                out.update(timed(ctx, lambda: net.rescale_output(x, MEAN, CFG)))
            else:
                xd = secdsrg.DeviceMaps.from_host(ctx, x)
                out.update(timed(ctx, lambda: net.rescale_output_dev(xd, MEAN, CFG).free()))
                xd.free()
        net.close()
    else:
        pred = secdsrg.Predictor("DSRG", weights, C, CFG, MEAN, size=(S, S), ctx=ctx)
        out.update(timed(ctx, lambda: pred.update(imgs, gts)))
        out["mIoU"] = pred.metrics()["mIoU"]
        pred.close()
    out["images_per_s"] = round(B / out["median_ms"] * 1e3, 1)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in STEPS:
        sys.exit("usage: python profiles/seg_predict.py {%s}" % " | ".join(STEPS))
    main(sys.argv[1])
