"""One SEC / DSRG training step (secdsrg.SegTrainer.step) at the reference's size: 321 x 321, 21 classes, the real widths (64 ... 512,
fc 1024; tests/deeplab_grad_ref.full_weights), f16x3, B images (argv[1], default 8: a tape of 8 x 199 MB for DSRG).

Prints one JSON line per method:
  step_ms                 wall time of one SegTrainer.step (the stream drained)
  forward_tape_ms         SegNet.forward_dev(keep=True)
  loss_chain_ms           SegNet.loss_step_dev minus a plain forward_dev: CRF layer, (DSRG) region growing, losses
  backward_ms             SegNet.backward_dev on the kept tape
  accumulate_ms, apply_ms, repack_ms   device-event time of wsc_seg_sgd_accumulate / _apply / wsc_net_seg_load_params, resident
                          buffers, with the HBM rate against their algorithmic bytes: accumulate 3 reads + 1 write of grad_elems
                          floats, apply 3 + 3, repack 2 reads of grad_elems floats + the packed rows of both planes + the rotated kernels
  rebuild_ms              the only way to updated weights in a net without the repack: SegGrads.to_host() (to_host_ms), then a new
                          SegNet and a new _lib.SegGrad from host weights (create_ms) -- host packing of both forms and two uploads
  repack_speedup          rebuild_ms / repack_ms

One GPU step per method; run it under its own time limit:   timeout -k 10 600 python profiles/seg_train_step.py [B]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import deeplab_grad_ref as gref  # noqa: E402
from tests import deeplab_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
C, HW, REPS = 21, (321, 321), 20
CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 5}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)

ctx = _lib.Context(0)


def wall(fn, reps=3):
    """ms per call, the stream drained before and after"""
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
        for d in (out if isinstance(out, tuple) else (out,)):
            if hasattr(d, "free"):
                d.free()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def device(fn, reps=REPS):
    for _ in range(3):
        fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


for method in ("DSRG", "SEC"):
    weights = gref.full_weights(method, C)
    rng = np.random.default_rng(5)
    x = DeviceMaps.from_host(ctx, ref.net_input(B, HW[0], HW[1], 12))
    tags = np.zeros((B, C), np.float32)
    tags[:, 0] = 1
    for b in range(B):
        tags[b, rng.choice(np.arange(1, C), 3, replace=False)] = 1
    tr = secdsrg.SegTrainer(method, weights, C, ctx=ctx, base_lr=1e-9)  # (a rate that keeps random weights in half's range)
    net, sg = tr.net, tr.net._grad
    h, w = net.map_size(*HW)
    cues = DeviceMaps.from_host(ctx, ((rng.random((B, h, w, C)) < 0.1) * tags[:, None, None, :]).astype(np.float32))
    E = sg.grad_elems

    def step():
        return tr.step(x, cues, tags, MEAN, CRF_CFG)[1] if method == "DSRG" else tr.step(x, cues, tags, MEAN, CRF_CFG)[0]

    step_ms = wall(step)
    fwd_tape_ms = wall(lambda: net.forward_dev(x, keep=True))
    fwd_ms = wall(lambda: net.forward_dev(x))
    loss_step = lambda: tuple(d for d in net.loss_step_dev(x, cues, tags, MEAN, CRF_CFG)[1:] if d is not cues)
    loss_ms = wall(loss_step) - fwd_ms
    prob, tape = net.forward_dev(x, keep=True)
    dfc8 = DeviceMaps.from_host(ctx, (1e-3 * rng.standard_normal(prob.shape)).astype(np.float32))
    bwd_ms = wall(lambda: net.backward_dev(tape, dfc8))
    grads = net.backward_dev(tape, dfc8)
    acc_ms = device(lambda: sg.sgd_accumulate(tr.params.ptr, grads.maps.ptr, tr.accum.ptr, 5e-4, 1, None))
    with DeviceMaps(ctx, (1,), np.float32) as l2:
        acc_l2_ms = device(lambda: sg.sgd_accumulate(tr.params.ptr, grads.maps.ptr, tr.accum.ptr, 5e-4, 1, l2.ptr))
    apply_ms = device(lambda: sg.sgd_apply(tr.params.ptr, tr.accum.ptr, tr.mom.ptr, 0.0, 0.9, True))
    repack_ms = device(lambda: sg.load_params(tr.params.ptr))
    planes = 2 * 2  # f16x3: hi and lo, 2 bytes each
    repack_bytes = E * (2 * 4 + planes + 4)

    t0 = time.perf_counter()
    host = grads.to_host()
    to_host_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    net2 = secdsrg.SegNet(method, weights, C, ctx=ctx)
    sg2 = _lib.SegGrad(net2.net, net2._sd)
    ctx.sync()
    create_ms = (time.perf_counter() - t0) * 1e3
    sg2.close()
    net2.close()
    del host
    for d in (prob, tape, dfc8, grads, x, cues):
        d.free()
    tr.close()
    gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)
    print(json.dumps({"method": method, "B": B, "size": HW, "classes": C, "grad_elems": E, "step_ms": round(step_ms, 2),
                      "forward_tape_ms": round(fwd_tape_ms, 2), "forward_ms": round(fwd_ms, 2), "loss_chain_ms": round(loss_ms, 2),
                      "backward_ms": round(bwd_ms, 2), "accumulate_ms": round(acc_ms, 4), "accumulate_l2_ms": round(acc_l2_ms, 4),
                      "apply_ms": round(apply_ms, 4), "repack_ms": round(repack_ms, 4), "accumulate_gbs": gbs(16 * E, acc_ms),
                      "accumulate_l2_gbs": gbs(16 * E, acc_l2_ms), "apply_gbs": gbs(24 * E, apply_ms), "repack_gbs": gbs(repack_bytes, repack_ms),
                      "to_host_ms": round(to_host_ms, 1), "create_ms": round(create_ms, 1), "rebuild_ms": round(to_host_ms + create_ms, 1),
                      "repack_speedup": round((to_host_ms + create_ms) / repack_ms, 1)}), flush=True)
