"""The backward pass of the IRNet heads at the reference's size: ResNet50, crop 512 (128 x 128 head maps), N = 16 and 32
(step/train_irn.py: irn_batch_size 32), f16x3 forward.

Prints one JSON line per batch size: the tape's size; device time (events, buffers resident) of wsc_net_forward_edge_raw, of
wsc_net_forward_edge_tape (the difference is what keeping the tape costs) and of wsc_net_backward_edge, the latter also per
kernel class (WscKernelTimer; the data-gradient convolutions run under the conv classes); and, on the same card, torch float32
autograd of the same heads on the tape's stage taps (oracle/irn_ref.py's _head ops: conv2d, group_norm, interpolate, relu),
forward + backward, as the comparison.  The gradient fed in is 1e-3 N(0, 1).

One GPU step; run it under its own time limit:   timeout -k 10 420 python profiles/irn_backward.py"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from oracle import irn_ref  # noqa: E402
from tests import irn_grad_ref as gref  # noqa: E402
from wsscam import _lib  # noqa: E402
from wsscam.net import resnet50_irn  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

S, REPS, TORCH_REPS = 512, 5, 3
ARCH = "resnet50"

sd = irn_ref.make_resnet50_irn_state_dict(seed=3)
m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=S, stride=4, precision=_lib.PREC_F16X3)
m.load_state_dict(sd)
m.eval().cuda(0)
ctx, net = m.ctx, m._ensure_net()
grad = m.irn_grad()
dev = torch.device("cuda:0")
names = sum(gref.param_names(ARCH), [])


def timed(fn, reps):
    fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


def torch_heads(xs, params, d_edge, d_dp):
    """Net.forward's heads on detached stage taps + backward, float32 on the device"""
    for p in params.values():
        p.grad = None
    heads = irn_ref.RESNET50_HEADS
    e = [irn_ref._head(xs[src - 1], params, n, st, g, up) for n, src, st, _, g, up in heads["edge"]]
    h2, w2 = e[1].shape[2], e[1].shape[3]
    edge = F.conv2d(torch.cat([e[0], e[1]] + [t[..., :h2, :w2] for t in e[2:]], dim=1), params["fc_edge6.weight"], params["fc_edge6.bias"])
    d = [irn_ref._head(xs[src - 1], params, n, st, g, up) for n, src, st, _, g, up in heads["dp"]]
    h3, w3 = d[2].shape[2], d[2].shape[3]
    up3 = irn_ref._head(torch.cat([d[2], d[3][..., :h3, :w3], d[4][..., :h3, :w3]], dim=1), params, "fc_dp6", 1, 16, 2)
    hid = irn_ref._head(torch.cat([d[0], d[1], up3[..., :d[1].shape[2], :d[1].shape[3]]], dim=1), params, "fc_dp7", 1, 16, 1)
    dp = F.conv2d(hid, params["fc_dp7.3.weight"])
    torch.autograd.backward([edge, dp], [d_edge, d_dp])


for N in (16, 32):
    rng = np.random.default_rng(N)
    x = rng.normal(0, 1, (N, 3, S, S)).astype(np.float32)
    entries, elems = net.edge_tape_plan(N, S)
    (He, We), (Hd, Wd) = net.edge_size(S)
    d_edge = (1e-3 * rng.standard_normal((N, He, We))).astype(np.float32)
    d_dp = (1e-3 * rng.standard_normal((N, 2, Hd, Wd))).astype(np.float32)
    xd, de, dd = (DeviceMaps.from_host(ctx, a) for a in (x, d_edge, d_dp))
    tape, out = DeviceMaps(ctx, (elems,), np.float32), DeviceMaps(ctx, (grad.grad_elems,), np.float32)
    edge, dp = DeviceMaps(ctx, (N, He, We), np.float32), DeviceMaps(ctx, (N, 2, Hd, Wd), np.float32)

    raw_ms = timed(lambda: net.forward_edge_raw(xd.ptr, N, S, edge.ptr, dp.ptr), REPS)
    tape_ms = timed(lambda: net.forward_edge_tape(xd.ptr, N, S, tape.ptr, elems, edge.ptr, dp.ptr), REPS)
    back_ms = timed(lambda: grad.backward(N, S, tape.ptr, elems, de.ptr, dd.ptr, out.ptr), REPS)
    ctx.profile_begin()
    grad.backward(N, S, tape.ptr, elems, de.ptr, dd.ptr, out.ptr)
    classes = {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in ctx.profile_end().items()}
    flat = out.to_host()

    # the same heads in torch float32 on the tape's taps
    by_name = {e["name"]: e for e in entries}
    xs = []
    for k in range(1, 6):
        e = by_name["x%d" % k]
        a = ctx.to_host(tape.buf, (N, e["Ho"], e["Wo"], e["C"]), np.float32, offset_bytes=4 * e["offset"])
        xs.append(torch.from_numpy(a).to(dev).permute(0, 3, 1, 2).contiguous())
    for mm in (xd, tape, edge, dp, out, de, dd):
        mm.free()
    params = {k: v.to(dev).requires_grad_(k in names) for k, v in sd.items() if k.startswith("fc_")}
    te, td = torch.from_numpy(d_edge).to(dev)[:, None], torch.from_numpy(d_dp).to(dev)
    for _ in range(2):
        torch_heads(xs, params, te, td)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(TORCH_REPS):
        torch_heads(xs, params, te, td)
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) / TORCH_REPS * 1e3
    # a sanity check that both sides compute the same thing (float32 autograd on an f16x3 tape's taps), not a parity claim
    off = next(e for e in grad.layout if e["name"] == "fc_dp7.0.weight")
    mine = flat[off["offset"]:off["offset"] + off["size"]].reshape(448, 256).T
    theirs = params["fc_dp7.0.weight"].grad[:, :, 0, 0].cpu().numpy()
    diff = float(np.abs(mine - theirs).max() / np.abs(theirs).max())
    assert diff <= 1e-2, diff
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    del xs, params, te, td
    torch.cuda.empty_cache()
    print(json.dumps({"N": N, "S": S, "precision": "f16x3", "tape_GB": round(4 * elems / 1e9, 3), "grad_floats": grad.grad_elems,
                      "forward_edge_raw_ms": round(raw_ms, 3), "forward_edge_tape_ms": round(tape_ms, 3),
                      "tape_extra_ms": round(tape_ms - raw_ms, 3), "backward_edge_ms": round(back_ms, 3), "backward_classes": classes,
                      "torch_f32_heads_fwd_bwd_ms": round(torch_ms, 2), "torch_peak_allocated_GiB": round(peak_gb, 2),
                      "fc_dp7.0.weight_max_diff_vs_torch_f32_rel": diff}))
