"""The SEC / DSRG prediction tail at VOC size: eight synthetic images of 375 x 500, C = 21, network maps of 321 x 321, the VOC
test configuration of the dense CRF (SEC.py:20).  Inputs of tests/helpers.synth_crf_case, ground truths of tests/seg_eval_ref.

Prints one JSON line:
  evaluator     images/s of secdsrg.SegEvaluator.update over the batch (wall clock; the call ends in a stream synchronisation)
  per_image     images/s of the only path there was before: per image misc.imutils.crf_inference on the resized map, numpy
                arg-max, the restated counting loop.  The map is resized OUTSIDE the timed window (cv2 is absent; the stand-in
                would be numpy), which favours this path.
  unary / argmax  kernel time of wsc_seg_unary_nhwc / wsc_seg_resize_argmax alone, buffers resident (device events), with the
                bytes they move (source read once + output written) over that time
Every timed figure: warm-up first, then REPS repeats, median and (min, max).

One GPU step; run it under its own time limit:   timeout -k 10 300 python profiles/seg_eval.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import helpers  # noqa: E402
from tests import seg_eval_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402
from wsscam.misc import imutils  # noqa: E402

B, H, W, C, h, w = 8, 375, 500, 21, 321, 321
CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 10}
WARM, REPS, KREPS = 2, 7, 50


def inputs():
    rng = np.random.default_rng(11)
    probs = [np.ascontiguousarray(np.transpose(helpers.synth_crf_case(rng, h, w, C)[2], (1, 2, 0)), dtype=np.float32) for _ in range(B)]
    images = [helpers.synth_crf_case(rng, H, W, 2)[0] for _ in range(B)]
    gts = [ref.gt_as_image(ref.make_gt_index(rng, H, W, C, absent=C - 2)) for _ in range(B)]
    return probs, images, gts


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    probs, images, gts = inputs()
    ctx = _lib.Context(0)

    ev = secdsrg.SegEvaluator(C, CFG, ctx=ctx)
    labels = ev.update(probs, images, gts, want_pred=True)
    for _ in range(WARM):
        ev.update(probs, images, gts)
    t_ev = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        ev.update(probs, images, gts)
        t_ev.append(time.perf_counter() - t0)
    ev.close()

    resized = [ref.resize_f64(p, (H, W)).astype(np.float32) for p in probs]  # outside the timed window

    def per_image():
        labs = []
        for b in range(B):
            labs.append(np.argmax(imutils.crf_inference(images[b], CFG, C, resized[b], use_log=True, ctx=ctx), axis=-1))
        return labs, ref.finish(ref.count_loop(labs, gts, C))

    for _ in range(WARM):
        labs, _ = per_image()
    agree = float(np.mean([np.mean(a == b) for a, b in zip(labs, labels)]))
    t_pi = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        per_image()
        t_pi.append(time.perf_counter() - t0)

    # the two kernels alone
    p_dev = ctx.to_device(np.concatenate([p.reshape(-1) for p in probs]))
    u_dev = ctx.alloc(B * C * H * W * 4)
    l_dev = ctx.alloc(B * H * W * 4)
    src, out = [(h, w)] * B, [(H, W)] * B
    s_off, u_off, l_off = (np.arange(B, dtype=np.int64) * n for n in (h * w * C, H * W * C, H * W))
    unary = lambda: _lib.seg_unary_nhwc(ctx, p_dev, C, src, out, s_off, u_off, u_dev)
    # (the softmax buffer read as class-major planes: the values do not matter for the time)
    argmax = lambda: _lib.seg_resize_argmax(ctx, p_dev, C, src, out, s_off, l_off, l_dev)
    kern = {}
    for name, fn, nbytes in (("unary", unary, 4.0 * B * C * (h * w + H * W)), ("argmax", argmax, 4.0 * B * (C * h * w + H * W))):
        for _ in range(10):
            fn()
        ms = []
        for _ in range(5):
            ctx.timer_begin()
            for _ in range(KREPS):
                fn()
            ms.append(ctx.timer_end() / KREPS)
        med, lo, hi = spread(ms)
        kern[name] = {"ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "bytes": nbytes,
                      "GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1)}

    e_med, e_lo, e_hi = spread(t_ev)
    p_med, p_lo, p_hi = spread(t_pi)
    print(json.dumps({"shape": {"B": B, "gt": [H, W], "map": [h, w], "C": C}, "reps": REPS,
                      "evaluator_images_per_s": round(B / e_med, 2), "evaluator_range": [round(B / e_hi, 2), round(B / e_lo, 2)],
                      "per_image_images_per_s": round(B / p_med, 2), "per_image_range": [round(B / p_hi, 2), round(B / p_lo, 2)],
                      "ratio": round(p_med / e_med, 3), "label_agreement": round(agree, 6), "kernels": kern}))


if __name__ == "__main__":
    main()
