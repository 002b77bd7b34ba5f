"""The 01_train batch stage at the workload's own size: B (argv[1], default 8) decoded VOC-sized images (synth.VOC_SIZES: 375 x 500,
500 x 375, ...) -> 321 x 321 network inputs, the VOC2012 training generator's draws (seeded), fill mode 'reflect'.

Prints one JSON line:
  kernel_ms               wsc_cls_train_batch alone, wsc_timer_* (device events on the ctx stream) around windows of REPS calls on
                          resident buffers, [median, min, max] over RUNS windows, per call -- with the warp ('warp') and with the
                          same flips but no warp ('direct'); bytes: the decoded source bytes in and 12 B H W out; GBps from the
                          median
  batcher_apply_wall_ms   ClsBatcher.apply (pack on the host, one upload, the kernel), host clock around a drained stream
  host_chain_ms           what the stage replaces, on the same decoded images and draws: PIL nearest resize, np.float32,
                          scipy.ndimage.affine_transform(order=1) per channel, flips, the fp32 standardisation, HWC -> CHW, per batch,
                          on one thread and on a pool of THREADS threads (decode excluded on both sides)
  trainer_step_wall_ms    ClsTrainer.step (VGG16 with BatchNorm, f16x3) on the batch the batcher made, the same clock; batch_share:
                          batcher_apply / (batcher_apply + step)

One GPU run; under its own time limit:   timeout -k 10 420 python profiles/cls_batch.py [B]"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from oracle import cnn_ref  # noqa: E402
from wsscam import _lib, cls_train, synth  # noqa: E402
from wsscam.net import vgg16_cam  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
S, C, REPS, RUNS, THREADS = 321, 20, 20, 5, 16

ctx = _lib.Context(0)
rng = np.random.default_rng(B)
images = [synth.synth_image(rng, *synth.VOC_SIZES[i % len(synth.VOC_SIZES)]) for i in range(B)]
aug = cls_train.ImageAugmenter.for_dataset("VOC2012", True)
batcher = cls_train.ClsBatcher(["-"] * B, np.zeros((B, C), np.float32), aug, S, B, False, 1, ctx=ctx)
_, affine, flags = batcher.plan()
sub, div, mul = aug.standardisation()
flat, offs, sizes = cls_train._pack_images(images)


def timed(fn):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(RUNS):
        ctx.timer_begin()
        for _ in range(REPS):
            fn()
        ms.append(ctx.timer_end() / REPS)
    return [round(float(np.median(ms)), 4), round(min(ms), 4), round(max(ms), 4)]


def wall(fn, reps=5):
    fn()
    ms = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)]


out = {"B": B, "S": S, "threads": THREADS, "bytes_in": int(flat.size), "bytes_out": 12 * B * S * S, "kernel_ms": {}, "kernel_GBps": {}}
with DeviceMaps.from_host(ctx, flat) as src, DeviceMaps(ctx, (B, 3, S, S), np.float32) as x:
    for name, fl in (("warp", flags), ("direct", flags & ~np.int32(1))):
        ms = timed(lambda: _lib.cls_train_batch(ctx, src.ptr, sizes, offs, (S, S), affine, fl, aug.fill_mode, aug.cval, sub, div, mul, x.ptr))
        out["kernel_ms"][name] = ms
        out["kernel_GBps"][name] = round((out["bytes_in"] + out["bytes_out"]) / ms[0] / 1e6, 1)
    got = x.to_host()  # (the last call: 'direct')


def apply_once():
    batcher.apply(images, affine, flags).free()


out["batcher_apply_wall_ms"] = wall(apply_once)


def host_sample(i, fl=None):
    f = int(flags[i] if fl is None else fl[i])
    img = np.asarray(Image.fromarray(images[i]).resize((S, S), Image.NEAREST), dtype=np.float32)
    if f & 1:
        m, off = affine[i, :4].reshape(2, 2), affine[i, 4:]
        img = np.stack([ndimage.affine_transform(img[:, :, c], m, off, order=1, mode=aug.fill_mode, cval=aug.cval) for c in range(3)], axis=2)
    if f & 2:
        img = img[:, ::-1]
    if f & 4:
        img = img[::-1]
    img = (img - sub.reshape(1, 1, 3)) / div
    img = img * mul
    return np.ascontiguousarray(img.transpose(2, 0, 1))


def host_wall(pool, reps=3):
    run = (lambda: list(pool.map(host_sample, range(B)))) if pool is not None else (lambda: [host_sample(i) for i in range(B)])
    run()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    return round((time.perf_counter() - t0) / reps * 1e3, 1)


out["host_chain_ms"] = {"1 thread": host_wall(None)}
with ThreadPoolExecutor(max_workers=THREADS) as pool:
    out["host_chain_ms"]["%d threads" % THREADS] = host_wall(pool)
want_direct = np.stack([host_sample(i, flags & ~np.int32(1)) for i in range(B)])
out["direct_bit_equal_to_host_chain"] = bool(np.array_equal(got.view(np.uint32), want_direct.view(np.uint32)))

model = vgg16_cam.CAM(None, "voc12", "", C, None, precision=_lib.PREC_F16X3)
model.load_state_dict(cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, True, seed=1))
model._ctx = ctx
targets = (np.random.default_rng(3).random((B, C)) < 0.3).astype(np.float32)
x = batcher.apply(images, affine, flags)
with x:
    out["warp_bit_equal_to_host_chain"] = bool(np.array_equal(x.to_host().view(np.uint32), np.stack([host_sample(i) for i in range(B)]).view(np.uint32)))
    with cls_train.ClsTrainer(model, "mean", C) as tr:
        out["trainer_step_wall_ms"] = wall(lambda: tr.step(x, targets, 0.0))
out["batch_share"] = round(out["batcher_apply_wall_ms"][0] / (out["batcher_apply_wall_ms"][0] + out["trainer_step_wall_ms"][0]), 4)
model._release_net()
ctx.sync()
print(json.dumps(out))
