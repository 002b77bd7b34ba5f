"""SEC / DSRG DeepLab-VGG16 forward pass with the tape and backward pass at the reference's size: 321 x 321 input, 41 x 41 maps,
21 classes, batch 4, f16x3 forward, He-scaled random weights at the real widths (tests/deeplab_ref.random_weights), every buffer
resident.  The backward pass is exact fp32 whatever the forward precision.

Prints one JSON object: per net the tape size, ms per batch of wsc_net_forward_seg, wsc_net_forward_seg_tape and
wsc_net_backward_seg (device events, wsc_timer_*), and the per-kernel-class split of one backward pass (wsc_profile_*: the
weight-gradient GEMMs with their algorithmic TFLOP/s, the data-gradient convolutions under the conv classes, the mask / bias /
pool kernels).  No time is asserted anywhere.

One GPU step; run it under its own time limit:   timeout -k 10 420 python profiles/seg_grad.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import deeplab_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

B, S, C, REPS, WARM = 4, 321, 21, 20, 2
WIDTHS = (64, 128, 256, 512, 512)

ctx = _lib.Context(0)
x_dev = DeviceMaps.from_host(ctx, ref.net_input(B, S, S, 5))
out = {"shape": [B, S, S, 3], "classes": C, "forward_precision": "f16x3", "reps": REPS, "nets": {}}


def timed(call):
    for _ in range(WARM):
        call()
    ctx.timer_begin()
    for _ in range(REPS):
        call()
    return round(ctx.timer_end() / REPS, 3)


for method in ("SEC", "DSRG"):
    weights = ref.random_weights(method, C, fc_width=1024, seed=21, widths=WIDTHS)
    net = secdsrg.SegNet(method, weights, C, precision=_lib.PREC_F16X3, ctx=ctx)
    prob, tape = net.forward_dev(x_dev, keep=True)
    dfc8 = DeviceMaps.from_host(ctx, (1e-3 * np.random.default_rng(3).standard_normal(prob.shape)).astype(np.float32))
    sg, elems = _lib.SegGrad(net.net, secdsrg.seg_state_dict(method, weights, C)), tape.shape[0]
    grads = secdsrg.SegGrads(DeviceMaps(ctx, (sg.grad_elems,), np.float32), sg.layout)
    sg.backward(B, S, S, tape.ptr, elems, dfc8.ptr, grads.maps.ptr)  # (allocates the workspace)
    first = grads.maps.to_host()
    assert np.isfinite(first).all() and np.abs(first).max() > 0
    ms_fwd = timed(lambda: net.net.forward_seg(x_dev.ptr, B, S, S, prob.ptr, None, 1e-4))
    ms_tape = timed(lambda: net.net.forward_seg_tape(x_dev.ptr, B, S, S, tape.ptr, elems, prob.ptr, None, 1e-4))
    ms_bwd = timed(lambda: sg.backward(B, S, S, tape.ptr, elems, dfc8.ptr, grads.maps.ptr))
    assert np.array_equal(first.view(np.uint32), grads.maps.to_host().view(np.uint32))  # every pass: the same bits
    ctx.profile_begin()
    sg.backward(B, S, S, tape.ptr, elems, dfc8.ptr, grads.maps.ptr)
    classes = {k: {"launches": v[0], "ms": round(v[1], 3), **({"tflops": round(v[2] / v[1] * 1e-9, 2)} if k.startswith(("wgrad", "conv")) else {})}
               for k, v in ctx.profile_end().items()}
    out["nets"][method] = {"tape_MB_per_image": round(elems * 4 / B / 1e6, 1), "grad_MB": round(sg.grad_elems * 4 / 1e6, 1),
                           "forward_ms": ms_fwd, "forward_tape_ms": ms_tape, "backward_ms": ms_bwd, "backward_classes": classes}
    for d in (prob, tape, dfc8, grads):
        d.free()
    sg.close()
    net.close()
x_dev.free()
print(json.dumps(out))
