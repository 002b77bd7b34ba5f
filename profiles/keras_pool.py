"""The max pool of a `pool_spec` at 3 x 3 / 2 SAME (launch_pool of csrc/pool.hip, through wsc_pool_tf_nhwc) on two tensors, f16x3:
  pool1   64 samples x 321 x 321 x 64   the VGG16 stack's first-pool tensor at the bench batch (32 images, [orig, flip])
  pool3   64 samples x  81 x  81 x 256  its third
The kernel time is the library's own per-class event timing (wsc_profile_*: the pool launch alone -- the entry's layout changes
carry no timer), CALLS launches per figure, REPS figures per tensor.

Then the VGG16 CAM stack at 321 x 321, 32 images, f16x3, with 3 x 3 / 2 SAME pools (41 x 41 maps) against the fixed architecture
(2 x 2 / 2, 40 x 40): wsc_net_forward_cam between device events, alternating.

Prints one JSON line.  One GPU step; run it under its own time limit:   timeout -k 10 420 python profiles/keras_pool.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from wsscam import _lib, synth  # noqa: E402
from wsscam.net import vgg16_cam  # noqa: E402

N, REPS, CALLS, PREC = 64, 5, 10, _lib.PREC_F16X3
TENSORS = {"pool1": (321, 321, 64), "pool3": (81, 81, 256)}

ctx = _lib.Context(0)
lib = ctx._lib


def fill(H, W, C, seed):
    """[N][H][W][C] float32 on the device: one sample's signed values, repeated"""
    one = (np.random.default_rng(seed).normal(0, 3, (H, W, C)) - 1.0).astype(np.float32)
    buf = ctx.alloc(N * one.nbytes)
    for n in range(N):
        _lib.check(lib.wsc_memcpy_h2d(ctx.h, buf.ptr + n * one.nbytes, one.ctypes.data, one.nbytes))
    ctx.sync()
    return buf


def pool_ms(call):
    """kernel time of one pool launch, the mean of CALLS launches"""
    ctx.profile_begin()
    for _ in range(CALLS):
        call()
    prof = ctx.profile_end()
    launches, ms, _ = prof["pool/layout/flip-add"]
    assert launches == CALLS and len(prof) == 1, prof
    return ms / CALLS


out = {"samples": N, "precision": "f16x3", "reps": REPS, "calls_per_rep": CALLS, "pools": {}}
for name, (H, W, C) in TENSORS.items():
    x_dev = fill(H, W, C, 7)
    Ho, Wo = -(-H // 2), -(-W // 2)
    y_tf = ctx.alloc(N * Ho * Wo * C * 4)
    tf = lambda: _lib.pool_tf_nhwc(ctx, x_dev, N, H, W, C, 3, 2, True, PREC, y_tf)  # noqa: E731
    tf()
    assert ctx.to_host(y_tf, (Ho * Wo * C,), np.float32).min() < 0  # (sample 0: signed values, the padding did not win)
    for _ in range(2):
        pool_ms(tf)
    t_tf = [pool_ms(tf) for _ in range(REPS)]
    planes = (N * H * W * C + N * Ho * Wo * C) * 4  # hi + lo, 2 bytes each, read + written
    out["pools"][name] = {"shape": [N, H, W, C], "bytes": planes, "pool_tf_ms": [round(v, 4) for v in t_tf],
                          "pool_tf_median_ms": round(float(np.median(t_tf)), 4), "pool_tf_spread_ms": round(max(t_tf) - min(t_tf), 4),
                          "pool_tf_TBps": round(planes / float(np.median(t_tf)) * 1e-9, 3)}
    for buf in (x_dev, y_tf):
        buf.free()

# the VGG16 CAM stack at the bench batch
B, S, C = 32, 321, 20
sd = synth.plain_state_dict("vgg16", C, True, seed=0)
x = np.random.default_rng(3).uniform(-0.5, 0.5, (B, 2, 3, S, S)).astype(np.float32)
models, bufs = {}, {}
for name, pooling in (("default_2x2_valid", None), ("same_3x3", [(3, 2, "same")] * 3)):
    m = vgg16_cam.CAM(None, "voc12", "", C, None, precision=PREC, pooling=pooling)
    m.load_state_dict(sd)
    m._ctx = ctx
    m.cuda(0)
    h = m.cam_size(S)
    models[name] = (m, h)
    bufs[name] = ctx.alloc(B * C * h * h * 4)
x_dev = ctx.to_device(x)


def stack_ms(name, calls=3):
    m, _ = models[name]
    ctx.timer_begin()
    for _ in range(calls):
        m.forward_batch_device(x_dev, B, S, bufs[name])
    return ctx.timer_end() / calls


for name in models:
    stack_ms(name, 2)
times = {name: [] for name in models}
for _ in range(REPS):
    for name in models:
        times[name].append(stack_ms(name))
out["vgg16_stack_321"] = {"images": B, "range_flag": ctx.range_status(clear=True)}
for name, (m, h) in models.items():
    out["vgg16_stack_321"][name] = {"cam": h, "ms": [round(v, 3) for v in times[name]], "median_ms": round(float(np.median(times[name])), 3)}
print(json.dumps(out))
