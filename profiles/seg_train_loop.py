"""The batch stage of a SEC / DSRG training iteration and the whole iteration at the reference's size: 321 x 321 input, 41 x 41 x 21
cues, the real widths (tests/deeplab_grad_ref.full_weights), f16x3, B = 8 decoded 375 x 500 images (argv[2], default 8), cue lists
of a tenth of the 41 x 41 pixels in three classes per image.  Method: argv[1], DSRG (default) or SEC.

Two paths to the same step inputs, alternated in one process (other work shares the host, so only figures of one call compare):
  device   secdsrg.SegBatcher.train_batch: one upload of the packed images, one wsc_seg_train_batch (lists in its staged table)
  host     what the package offered before: numpy densify and label on the host, a DeviceMaps.from_host upload of the dense cues
           (141 KB per image), SegNet.preprocess_dev; the labels travel in SegTrainer.step
Prints one JSON line:
  batch_ms   {path: [median, min, max]} over RUNS windows of REPS batch stages, host clock, the stream drained at both ends
  iter_ms    the same for batch stage + SegTrainer.step (what SegTrainLoop runs per iteration, the files already decoded)
  cue_bytes_uploaded   per batch, either path

One GPU step per invocation; run it under its own time limit:   timeout -k 10 600 python profiles/seg_train_loop.py DSRG [B]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import deeplab_grad_ref as gref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

METHOD = sys.argv[1] if len(sys.argv) > 1 else "DSRG"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
C, HW, S = 21, (321, 321), 41
WARM, REPS, RUNS, ITER_REPS = 3, 20, 5, 3
CRF_CFG = secdsrg.CRF_CONFIG_TRAIN
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)

ctx = _lib.Context(0)
rng = np.random.default_rng(7)
ids = ["im%d" % b for b in range(B)]
images = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in ids]
cues_data = {}
for i in ids:
    classes = np.concatenate(([0], rng.choice(np.arange(1, C), 2, replace=False)))
    n = S * S // 10
    cues_data[i + "_cues"] = np.stack([rng.choice(classes, n), rng.integers(0, S, n), rng.integers(0, S, n)])
    cues_data[i + "_labels"] = classes[1:]

tr = secdsrg.SegTrainer(METHOD, gref.full_weights(METHOD, C), C, ctx=ctx, base_lr=1e-9)  # (a rate that keeps random weights in half's range)
batcher = secdsrg.SegBatcher(C, MEAN, size=HW, seed_size=S, ctx=ctx)


def batch_device():
    return batcher.train_batch(ids, images, cues_data)


def batch_host():
    labels = np.zeros((B, C), np.float32)
    cues = np.zeros((B, S, S, C), np.float32)
    for b, i in enumerate(ids):
        labels[b, cues_data[i + "_labels"]] = 1.0
        labels[b, 0] = 1.0
        c = cues_data[i + "_cues"]
        cues[b, c[1], c[2], c[0]] = 1.0
    cd = DeviceMaps.from_host(ctx, cues)
    try:
        return tr.net.preprocess_dev(images, MEAN, HW), cd, labels
    except Exception:
        cd.free()
        raise


def free(out):
    for d in out:
        if hasattr(d, "free"):
            d.free()


def iteration(batch):
    x, cues, labels = out = batch()
    try:
        new_cues = tr.step(x, cues, labels, MEAN, CRF_CFG)[1]
        if new_cues is not cues:
            new_cues.free()
    finally:
        free(out)


def window(fn, reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def alternate(fns, reps):
    """{name: [median, min, max] ms} over RUNS windows per path, the paths taking turns"""
    for fn in fns.values():
        for _ in range(WARM if reps > ITER_REPS else 1):
            fn()
    got = {k: [] for k in fns}
    for _ in range(RUNS):
        for k, fn in fns.items():
            got[k].append(window(fn, reps))
    return {k: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)] for k, v in got.items()}


# the two paths give the same step inputs
dev, host = batch_device(), batch_host()
same = [bool(np.array_equal(d.to_host(), h.to_host() if hasattr(h, "to_host") else h)) for d, h in zip(dev, host)]
free(dev)
free(host)
if not all(same):
    raise SystemExit("the two paths disagree: x, cues, labels equal = %r" % (same,))

batch_ms = alternate({"device": lambda: free(batch_device()), "host": lambda: free(batch_host())}, REPS)
iter_ms = alternate({"device": lambda: iteration(batch_device), "host": lambda: iteration(batch_host)}, ITER_REPS)
tr.close()
print(json.dumps({"method": METHOD, "B": B, "size": HW, "seed_size": S, "classes": C, "windows": RUNS, "batch_reps": REPS, "iter_reps": ITER_REPS,
                  "batch_ms": batch_ms, "iter_ms": iter_ms,
                  "cue_bytes_uploaded": {"device": int(sum(12 * cues_data[i + "_cues"].shape[1] for i in ids)), "host": B * S * S * C * 4}}),
      flush=True)
