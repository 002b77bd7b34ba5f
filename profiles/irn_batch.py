"""The IRNet training batch at the workload's own size: B = 32 samples of VOC size (375 x 500 and the other sizes of
synth.VOC_SIZES), crop 512, factors spread over 0.5 .. 1.5, random flips and crop boxes (seeded).

Prints one JSON line:
  batcher_apply_wall_ms   irn_train.TrainBatcher.apply (pack on the host, two uploads, wsc_irn_train_batch), host clock around a
                          drained stream, REPS repeats after one warm-up call; batcher_kernels: the context profiler's record of
                          one call ({class: (launches, ms, bytes)}: both kernels are timed under the pool / layout class, so
                          their sum is what it gives); batcher_pack_upload_wall_ms: the host pack and the two uploads alone
  host_chain_ms           the host datasets' item() on the same decoded samples and records -- PIL rescale, normalise, flip,
                          crop, reduce -- per batch, on one thread and on a pool of THREADS threads (decode excluded on both
                          sides: it stays on the host either way)
  trainer_step_wall_ms    IrnTrainer.step (ResNet50, f16x3, PathIndex(10)) on the batch the batcher made, the same clock

One GPU run; under its own time limit:   timeout -k 10 420 python profiles/irn_batch.py"""
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from wsscam import _lib, irn_train, synth  # noqa: E402
from wsscam.misc.indexing import PathIndex  # noqa: E402
from wsscam.net import resnet50_irn  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402
from wsscam.voc12.dataloader import AffinityDatasetMixin, SegmentationDatasetBase  # noqa: E402

B, S, REPS, THREADS = 32, 512, 5, 8


class MemoryDataset(AffinityDatasetMixin, SegmentationDatasetBase):
    """the VOC transform on samples that are already decoded"""

    def __init__(self, data, **kw):
        super().__init__(None, S, **kw)
        self.data, self.img_name_list = data, list(range(len(data)))

    def decoded(self, idx):
        return self.data[idx]


rng = np.random.default_rng(B)
data = []
for i in range(B):
    h, w = synth.VOC_SIZES[i % len(synth.VOC_SIZES)]
    data.append((synth.synth_image(rng, h, w), rng.choice(np.array([0, 5, 20, 21, 255], np.uint8), (h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w].copy()))
ds = MemoryDataset(data, rescale=(0.5, 1.5), norm_mode="float", hor_flip=True, crop_method="random")
random.seed(B)
factors = np.linspace(0.5, 1.5, B)
params = []
for i, f in enumerate(factors):  # the dataset's draw with the factor pinned to the spread
    ds.rescale = (float(f), float(f))
    params.append(ds.draw(i, data[i][0].shape[:2]))
params = np.stack(params)

sd = synth.irn_state_dict("resnet50", seed=0)
m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=S, stride=4, precision=_lib.PREC_F16X3)
m.load_state_dict(sd)
m.eval().cuda(0)
ctx = m.ctx
batcher = irn_train.TrainBatcher(ctx, S, "float")
images, labels = [d[0] for d in data], [d[1] for d in data]


def wall(fn, reps):
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def apply_once():
    for mp in batcher.apply(images, labels, params):
        mp.free()


def pack_upload():
    img = batcher._pack("image", images, 3)[0]
    lab = batcher._pack("label", labels, 2)[0]
    DeviceMaps.from_host(ctx, img).free()
    DeviceMaps.from_host(ctx, lab).free()


out = {"B": B, "S": S, "threads": THREADS, "scaled_sizes": [params[0][:2].tolist(), params[-1][:2].tolist()],
       "decoded_MB": round(sum(i.nbytes + l.nbytes for i, l in data) / 1e6, 2), "x_MB": round(B * 3 * S * S * 4 / 1e6, 2)}
out["batcher_apply_wall_ms"] = round(wall(apply_once, REPS), 3)
out["batcher_pack_upload_wall_ms"] = round(wall(pack_upload, REPS), 3)
ctx.profile_begin()
apply_once()
out["batcher_kernels"] = {k: (v[0], round(v[1], 4), v[2]) for k, v in ctx.profile_end().items()}


def host_chain(pool):
    run = (lambda i: ds.item(i, params[i], data[i]))
    return list(pool.map(run, range(B))) if pool is not None else [run(i) for i in range(B)]


def host_wall(pool, reps=3):
    host_chain(pool)
    t0 = time.perf_counter()
    for _ in range(reps):
        host_chain(pool)
    return (time.perf_counter() - t0) / reps * 1e3


out["host_chain_ms"] = {"1 thread": round(host_wall(None), 1)}
with ThreadPoolExecutor(max_workers=THREADS) as pool:
    out["host_chain_ms"]["%d threads" % THREADS] = round(host_wall(pool), 1)
items = host_chain(None)

x, label, reduced = batcher.apply(images, labels, params)
with x, label, reduced:
    out["bit_equal_to_host_chain"] = bool(np.array_equal(x.to_host().view(np.uint32), np.stack([it["img"] for it in items]).view(np.uint32))
                                          and np.array_equal(reduced.to_host(), np.stack([it["reduced_label"] for it in items])))
    with irn_train.IrnTrainer(m, PathIndex(10), 0.1, 1e-4, 1000) as tr:
        out["trainer_step_wall_ms"] = round(wall(lambda: tr.step(x, reduced), REPS), 3)
m._release_net()
print(json.dumps(out))
