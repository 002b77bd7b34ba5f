"""The 02_cues seed stage at the VOC batch of 02_cues/demo.py:643-664: B = 8 images, 41 x 41 seeds, C = 20 classes for both the
foreground and the background model, from Grad-CAM maps that are resident on the device (synthetic NHWC stacks at the VGG16
grid of a 321 x 321 input, 41 x 41: ReLU of N(0.1, 1), a third of the classes gated on).

Prints one JSON line, per batch:
  kernel_ms        wsc_cue_maps x 2 + wsc_cue_seeds, device events, every buffer resident (wsc_timer_*)
  device_wall_ms   the stage as gen_cues(device_seeds=True) runs it: two gate uploads, the three calls, the label bytes back
  host_wall_ms     the stage as gen_cues runs it by default (the parent commit's only path): both stacks to the host, the float64
                   gate, transpose, resize_stack (upload + wsc_bilinear_resize + download) x 2, cues.get_fgbg_cues
The device labels are checked against tests/cue_seeds_ref.seeds on the maps the host path forms.

One GPU step; run it under its own time limit:   timeout -k 10 180 python profiles/cue_seeds.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import cue_seeds_ref  # noqa: E402
from wsscam import _lib  # noqa: E402
from wsscam.cues import utilities as cu  # noqa: E402

B, h, C, S, THRESH, REPS = 8, 41, 20, 41, 0.2, 200

ctx = _lib.Context(0)
rng = np.random.default_rng(11)
cams = {m: np.maximum(rng.normal(0.1, 1.0, (B, h, h, C)), 0).astype(np.float32) for m in ("fg", "bg")}
gate = {m: (rng.random((B, C)) < 1 / 3).astype(np.float32) for m in ("fg", "bg")}
chan = np.arange(C)
cams_dev = {m: ctx.to_device(cams[m]) for m in cams}
gate_dev = {m: ctx.to_device(gate[m]) for m in cams}
maps_dev = {m: ctx.alloc(B * C * S * S * 4) for m in cams}
lab_dev = ctx.alloc(B * S * S)


def kernels(gates):
    for m in ("fg", "bg"):
        _lib.cue_maps(ctx, cams_dev[m], B, h, h, C, chan, gates[m], S, maps_dev[m])
    _lib.cue_seeds(ctx, maps_dev["fg"], maps_dev["bg"], B, C, C, S, S, THRESH, lab_dev)


def device_stage():
    up = {m: ctx.to_device(gate[m], pooled=True) for m in ("fg", "bg")}
    kernels(up)
    labels = ctx.to_host(lab_dev, (B, S, S), np.uint8)
    for buf in up.values():
        buf.free()
    return labels


def host_stage():
    H = {}
    for m in ("fg", "bg"):
        x = ctx.to_host(cams_dev[m], (B, h, h, C), np.float32)
        x = x[:, :, :, chan].astype(np.float64) * gate[m][:, None, None, :]
        H[m] = cu.resize_stack(np.transpose(x, (0, 3, 1, 2)), (S, S), ctx=ctx)
    return cu.get_fgbg_cues({}, H["fg"], H["bg"], [None] * B, list(range(B)), THRESH), H


cues, H = host_stage()
want, _, ambiguous = cue_seeds_ref.seeds(H["fg"].astype(np.float32), H["bg"].astype(np.float32), THRESH)
for _ in range(10):
    assert np.array_equal(device_stage(), want)
host_lab = cue_seeds_ref.labels_from_cues(cues, range(B), S, S)
assert np.array_equal(host_lab[~ambiguous], want[~ambiguous])

ctx.timer_begin()
for _ in range(REPS):
    kernels(gate_dev)
kernel_ms = ctx.timer_end() / REPS

t0 = time.perf_counter()
for _ in range(REPS):
    device_stage()
device_ms = (time.perf_counter() - t0) / REPS * 1e3

for _ in range(10):
    host_stage()
t0 = time.perf_counter()
for _ in range(REPS):
    host_stage()
host_ms = (time.perf_counter() - t0) / REPS * 1e3

print(json.dumps({"shape": [B, C, C, S, S], "cam_grid": [h, h], "seed_pixels": int((want != 0).sum()),
                  "background_pixels": int((want == 1).sum()), "ambiguous_pixels": int(ambiguous.sum()), "reps": REPS,
                  "kernel_ms_per_batch": round(kernel_ms, 4), "device_wall_ms_per_batch": round(device_ms, 4),
                  "host_wall_ms_per_batch": round(host_ms, 3)}))
