"""SEC / DSRG DeepLab-VGG16 forward pass at the reference's size: 321 x 321 input, 41 x 41 maps, 21 classes, batch 16 (an
assumption: the reference takes its batch size from the command line), f16x3, He-scaled random weights at the real widths
(tests/deeplab_ref.random_weights), input and output buffers resident.

Prints one JSON line:
  nets    wsc_net_forward_seg of DSRG (four ASPP branches) and SEC (one branch): ms per batch (device events, wsc_timer_*) and
          images/s, plus the per-kernel-class split of one batch (wsc_profile_*)
  layers  every dilated layer of the nets through wsc_conv2d_nchw_dil at its real shape (N = 16, 41 x 41; conv5_x 512 -> 512
          at rate 2, fc6 512 -> 1024 at rates 6 / 12 / 18 / 24): conv kernel time (the profile's conv classes: layout changes
          and weight packing are not in it), next to the SAME layer at dil = 1, pad = 1 on the same generic kernel variant
          (WSC_CONV_GENERIC) and on the variant the host picks for an undilated layer (FAST epilogue, LDS input window).
The comparison that matters is dilated vs undilated on the same kernel: the taps gather the same number of bytes, so a large
gap would mean the dilated path lost its staging.

One GPU step; run it under its own time limit:   timeout -k 10 300 python profiles/deeplab_seg.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import deeplab_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402

B, S, C, REPS, WARM = 16, 321, 21, 10, 3
WIDTHS = (64, 128, 256, 512, 512)
PREC = _lib.PREC_F16X3

ctx = _lib.Context(0)
x = ref.net_input(B, S, S, 5)
x_dev = ctx.to_device(x)
out = {"shape": [B, S, S, 3], "classes": C, "precision": "f16x3", "reps": REPS, "nets": {}, "layers": []}

for method in ("DSRG", "SEC"):
    net = secdsrg.SegNet(method, ref.random_weights(method, C, fc_width=1024, seed=21, widths=WIDTHS), C, precision=PREC, ctx=ctx)
    h, w = net.map_size(S, S)
    p_dev = ctx.alloc(B * h * w * C * 4)
    call = lambda: net.net.forward_seg(x_dev, B, S, S, p_dev, None, 1e-4)
    for _ in range(WARM):
        call()
    assert ctx.range_status(clear=True) == 0, "the He-scaled net left half's range"
    prob = ctx.to_host(p_dev, (B, h, w, C), np.float32)
    assert np.isfinite(prob).all() and np.abs(prob.sum(-1) - 1).max() < 1e-5
    ctx.timer_begin()
    for _ in range(REPS):
        call()
    ms = ctx.timer_end() / REPS
    ctx.profile_begin()
    call()
    classes = {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in ctx.profile_end().items()}
    out["nets"][method] = {"map": [h, w], "ms_per_batch": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1), "classes": classes}
    p_dev.free()
    net.close()
x_dev.free()


def conv_ms(xl_dev, wl, dil, pad, prec):
    """conv kernel time of one wsc_conv2d_nchw[_dil] call: the median of REPS profiled calls"""
    y_dev = ctx.alloc(B * wl.shape[0] * 41 * 41 * 4)
    ms = []
    for i in range(WARM + REPS):
        ctx.profile_begin()
        _lib.conv2d_nchw(ctx, xl_dev, B, wl.shape[1], 41, 41, wl, 1, pad, None, None, None, True, prec, y_dev, dil=dil)
        t = sum(v[1] for k, v in ctx.profile_end().items() if k.startswith("conv"))
        if i >= WARM:
            ms.append(t)
    y_dev.free()
    return float(np.median(ms))


rng = np.random.default_rng(3)
xl = np.maximum(rng.normal(0, 1, (B, 512, 41, 41)), 0).astype(np.float32)
xl_dev = ctx.to_device(xl)
for name, cout, rates in (("conv5_x", 512, (2,)), ("fc6", 1024, (6, 12, 18, 24))):
    wl = (rng.normal(0, 1, (cout, 512, 3, 3)) * np.sqrt(2.0 / (512 * 9))).astype(np.float32)
    same = conv_ms(xl_dev, wl, 1, 1, PREC | _lib.CONV_GENERIC)
    picked = conv_ms(xl_dev, wl, 1, 1, PREC)
    gflop = 2.0 * B * 41 * 41 * cout * 512 * 9 / 1e9
    for r in rates:
        d = conv_ms(xl_dev, wl, r, r, PREC)
        out["layers"].append({"layer": name, "cin": 512, "cout": cout, "dil": r, "dilated_ms": round(d, 4),
                              "dil1_same_kernel_ms": round(same, 4), "dil1_picked_variant_ms": round(picked, 4),
                              "dilated_over_same_kernel": round(d / same, 3), "gflop": round(gflop, 2),
                              "dilated_tflops": round(gflop / d, 1)})
xl_dev.free()
print(json.dumps(out))
