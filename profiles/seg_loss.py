"""The SEC / DSRG loss head at the reference's size: 41 x 41 x 21 (model.py:35), B = 16 (an assumption: the reference takes its
batch size from the command line), inputs of tests/seg_loss_ref.make_case.

Prints one JSON line per method: kernel time of wsc_seg_loss (device events, buffers resident) without a gradient, with
d loss / d fc8 and with both gradients; wall time of secdsrg.SegLoss on device maps (call + download of the nine loss values); and
the same step done on the host: download of the three maps + a vectorised numpy float64 restatement (host_step below: losses and
d loss / d fc8).  The reference runs this node inside its TensorFlow graph in float32; that cannot run here and no figure for it
is claimed.

One GPU step; run it under its own time limit:   timeout -k 10 180 python profiles/seg_loss.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import seg_loss_ref as ref  # noqa: E402
from wsscam import _lib, secdsrg  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

B, H, W, C, REPS, M = 16, 41, 41, 21, 200, 1e-4
N = H * W
LAUNCHES = {"SEC": "4 with a gradient (rank, pixel, finish, grad), 3 without; + one copy of the two weight tables",
            "DSRG": "3 with a gradient (pixel, finish, grad), 2 without"}


def host_step(method, p32, crf32, cues32, labels, tables):
    """numpy float64: the losses' sum and d loss / d fc8, the formulas of include/wsscam.h"""
    p, q, cues = p32.astype(np.float64), np.exp(crf32.astype(np.float64)), cues32.astype(np.float64)
    m = float(np.float32(M))
    if method == "SEC":
        cnt = np.maximum(cues.sum((1, 2, 3), keepdims=True), 1e-5)
        loss = -((cues * np.log(p)).sum((1, 2, 3)) / cnt.reshape(-1)).mean() + (q * np.log(q / p)).sum() / (B * N)
        g = -cues / cnt / p / B - q / p / (B * N)
        w_fg, z_fg, w_bg, z_bg = tables
        maps = p.reshape(B, N, C)
        order = np.argsort(p32.reshape(B, N, C), axis=1, kind="stable")
        srt = np.take_along_axis(maps, order, 1)
        w = np.concatenate([np.broadcast_to((w_bg / z_bg)[:, None], (N, 1)), np.broadcast_to((w_fg / z_fg)[:, None], (N, C - 1))], 1)
        mean = (srt * w[None]).sum(1)  # (B, C)
        stat = labels[:, 1:] > 0
        pos, neg = np.maximum(stat.sum(1, keepdims=True), 1e-5), np.maximum((~stat).sum(1, keepdims=True), 1e-5)
        vmax = maps[:, :, 1:].max(1)
        loss += -(np.where(stat, np.log(mean[:, 1:]), 0.0) / pos).sum(1).mean() - np.log(mean[:, 0]).mean() \
            - (np.where(stat, 0.0, np.log(1 - vmax)) / neg).sum(1).mean()
        coeff = np.concatenate([np.ones((B, 1)), stat / pos], 1)  # (B, C)
        ge = np.empty_like(maps)
        np.put_along_axis(ge, order, np.broadcast_to(w[None], maps.shape) * (-coeff / mean / B)[:, None, :], 1)
        at_max = maps[:, :, 1:] == vmax[:, None, :]
        ge[:, :, 1:] += at_max * ((~stat) / neg / (1 - vmax) / at_max.sum(1) / B)[:, None, :]
        g = g + ge.reshape(p.shape)
    else:
        loss, g = 0.0, np.zeros_like(p)
        for sl in (slice(0, 1), slice(1, None)):
            cnt = cues[..., sl].sum((1, 2, 3), keepdims=True) + 1e-8
            loss += -((cues[..., sl] * np.log(p[..., sl])).sum((1, 2, 3)) / cnt.reshape(-1)).mean()
            g[..., sl] = -cues[..., sl] / cnt / p[..., sl] / B
        pe = p + 1e-8
        ratio = q / pe
        loss += (q * np.log(ratio + 1e-8)).sum() / (B * N)
        g -= q * (ratio / pe) / (ratio + 1e-8) / (B * N)
    s = p * (1 + C * m) - m
    return loss, s * (g - (g * s).sum(3, keepdims=True)) / (1 + C * m)


ctx = _lib.Context(0)
prob, crf, cues, labels = ref.make_case((B, H, W, C))
tables = tuple(np.float64(v) for v in secdsrg.rank_weights(N, secdsrg.SEC_Q_FG) + secdsrg.rank_weights(N, secdsrg.SEC_Q_BG))
w_fg, z_fg = secdsrg.rank_weights(N, secdsrg.SEC_Q_FG)
w_bg, z_bg = secdsrg.rank_weights(N, secdsrg.SEC_Q_BG)
p_dev, q_dev, c_dev, l_dev = (DeviceMaps.from_host(ctx, a) for a in (prob, crf, cues, labels))
loss_dev = DeviceMaps(ctx, (len(_lib.SEG_LOSS_SLOTS),), np.float64)
gp_dev, gz_dev = DeviceMaps(ctx, prob.shape, np.float32), DeviceMaps(ctx, prob.shape, np.float32)

for method, code in (("SEC", _lib.SEG_LOSS_SEC), ("DSRG", _lib.SEG_LOSS_DSRG)):
    sec = method == "SEC"

    def call(gp=None, gz=None):
        _lib.seg_loss(ctx, code, p_dev.ptr, q_dev.ptr, c_dev.ptr, l_dev.ptr if sec else None, B, H, W, C, M, w_fg if sec else None, z_fg,
                      w_bg if sec else None, z_bg, loss_dev.ptr, grad_prob_dev=gp, grad_fc8_dev=gz)

    kernel_ms = {}
    for name, kw in (("loss_only", {}), ("with_grad_fc8", {"gz": gz_dev.ptr}), ("with_both_grads", {"gp": gp_dev.ptr, "gz": gz_dev.ptr})):
        for _ in range(10):
            call(**kw)
        ctx.timer_begin()
        for _ in range(REPS):
            call(**kw)
        kernel_ms[name] = round(ctx.timer_end() / REPS, 4)
    want_loss, want_gz = host_step(method, prob, crf, cues, labels, tables)
    got_gz = gz_dev.to_host()
    assert abs(loss_dev.to_host()[6] - want_loss) <= 1e-9 * abs(want_loss)
    assert np.abs(got_gz - want_gz).max() <= 1e-6 * np.abs(want_gz).max()

    sl = secdsrg.SegLoss(method, C, min_prob=M, ctx=ctx)

    def step():
        losses, g = sl(p_dev, q_dev, c_dev, labels=l_dev, want_grad="fc8")
        g.free()
        return losses

    for _ in range(10):
        step()
    t0 = time.perf_counter()
    for _ in range(REPS):
        step()
    wall_ms = (time.perf_counter() - t0) / REPS * 1e3

    def host():
        return host_step(method, p_dev.to_host(), q_dev.to_host(), c_dev.to_host(), labels, tables)

    host()
    t0 = time.perf_counter()
    for _ in range(5):
        host()
    host_ms = (time.perf_counter() - t0) / 5 * 1e3
    print(json.dumps({"method": method, "shape": [B, H, W, C], "reps": REPS, "kernel_ms_per_call": kernel_ms,
                      "segloss_wall_ms_per_call": round(wall_ms, 4), "download_plus_numpy_ms_per_call": round(host_ms, 2),
                      "launches_per_call": LAUNCHES[method]}))
