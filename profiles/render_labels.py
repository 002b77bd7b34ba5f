"""The debug-image renderer at the reference's ADP size: B (argv[1], default 16) label maps of S x S (argv[2], default 224) -> 1088 x 1088
colour images and overlays, 28 colours (ADP-morph without its background), OVERLAY_R = 0.75, one wsc_render_labels launch.

Prints one JSON line:
  kernel_ms     wsc_render_labels alone, wsc_timer_* (device events on the ctx stream) around windows of REPS calls on resident
                buffers, [median, min, max] over RUNS windows, per call -- 'overlay' (image in, colour image and overlay out: 9 bytes
                per pixel) and 'colour' (overlay_dev = NULL: 3 bytes per pixel); the label bytes read are added to `bytes`
  kernel_GBps   bytes / the median, to be read next to the 6.3 TB/s a streaming kernel reaches on this part.  WARM: a window renders
                the same 174 MB twenty times, less than the part's 256 MB last-level cache
  cold_ms       ONE launch with the overlay between device events, after a 1 GB buffer has been set (whatever of the working set
                the cache held is gone), [median, min, max] over COLD_RUNS such launches; cold_GBps from the median
  host_loop_ms  the reference's literal loop for the same batch on this host, one thread, per batch: per image and class
                `pred_segmask += (pred_idx == k)[..., None] * colour` on a float64 (H, W, 3) array, np.uint8, and the float64 blend
                (tests/render_ref.py; the nearest resize included, PNG encoding excluded on both sides), over HOST_IMAGES images
                scaled to B
  equal         the launch's bytes against that loop's on the first HOST_IMAGES images

One GPU run; under its own time limit:   timeout -k 10 420 python profiles/render_labels.py [B] [S]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import render_ref  # noqa: E402
from wsscam import _lib, render  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
S = int(sys.argv[2]) if len(sys.argv) > 2 else 224
OUT, N_COLOURS, R, REPS, RUNS, HOST_IMAGES, COLD_RUNS = 1088, 28, 0.75, 20, 5, 2, 7

ctx = _lib.Context(0)
rng = np.random.default_rng(B)
palette = np.asarray(render.colours_for("ADP-morph")[1:], np.uint8)
assert len(palette) == N_COLOURS
labels = rng.integers(0, N_COLOURS + 1, (B, S, S)).astype(np.int32)  # (one value in 29 is unlisted)
labels = np.repeat(np.repeat(labels[:, ::8, ::8], 8, axis=1), 8, axis=2)[:, :S, :S].copy()  # blobs, as a CRF's label map has them
images = rng.integers(0, 256, (B, OUT, OUT, 3)).astype(np.uint8)
npix = OUT * OUT
out_off = np.arange(B, dtype=np.int64) * 3 * npix
lab_off = np.arange(B, dtype=np.int64) * S * S
lab_dev, img_dev = ctx.to_device(labels), ctx.to_device(images)
colour_dev, overlay_dev = ctx.alloc(3 * npix * B), ctx.alloc(3 * npix * B)
blend = render.blend_table(palette, (0, 0, 0), R)
pal, other = render.palette_bytes(palette, (0, 0, 0))


def launch(with_overlay):
    _lib.render_labels(ctx, lab_dev, np.int32, [(S, S)] * B, [(OUT, OUT)] * B, lab_off, out_off, pal, other, colour_dev,
                       img_dev=img_dev if with_overlay else None, blend=blend if with_overlay else None,
                       overlay_dev=overlay_dev if with_overlay else None)


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


out = {"B": B, "S": S, "out": OUT, "n_colours": N_COLOURS, "kernel_ms": {}, "bytes": {}, "kernel_GBps": {}}
for name, with_overlay in (("overlay", True), ("colour", False)):
    ms = timed(lambda: launch(with_overlay))
    out["kernel_ms"][name] = ms
    out["bytes"][name] = B * (npix * (9 if with_overlay else 3) + 4 * S * S)
    out["kernel_GBps"][name] = round(out["bytes"][name] / ms[0] / 1e6, 1)
flush = ctx.alloc(1 << 30)
cold = []
for _ in range(COLD_RUNS):
    _lib.check(ctx._lib.wsc_memset(ctx.h, flush.ptr, 0, 1 << 30))
    ctx.sync()
    ctx.timer_begin()
    launch(True)
    cold.append(ctx.timer_end())
flush.free()
out["cold_ms"] = [round(float(np.median(cold)), 4), round(min(cold), 4), round(max(cold), 4)]
out["cold_GBps"] = round(out["bytes"]["overlay"] / out["cold_ms"][0] / 1e6, 1)
launch(True)
got_c = ctx.to_host(colour_dev, (B, OUT, OUT, 3), np.uint8)
got_o = ctx.to_host(overlay_dev, (B, OUT, OUT, 3), np.uint8)

t0 = time.perf_counter()
want = [render_ref.render(labels[b], palette, (OUT, OUT), img=images[b], overlay_r=R) for b in range(HOST_IMAGES)]
out["host_loop_ms"] = round((time.perf_counter() - t0) * 1e3 * B / HOST_IMAGES, 1)
out["equal"] = bool(all(np.array_equal(got_c[b], w[0]) and np.array_equal(got_o[b], w[1]) for b, w in enumerate(want)))
ctx.sync()
print(json.dumps(out))
