"""One IRNet training step at the reference's size: ResNet50, crop 512 (128 x 128 head maps), N = 16, f16x3 forward,
PathIndex(radius=10) -- irn_train.IrnTrainer.step split into its five device parts, and the same step done the only way that
was open before the update ran on the device.

Prints one JSON line:
  device parts (events, buffers resident, REPS repeats after one warm-up call): wsc_net_forward_edge_tape, wsc_irn_aff_loss,
      wsc_net_backward_edge, wsc_irn_sgd_step, wsc_net_irn_load_params
  trainer_step_wall_ms     IrnTrainer.step on a resident input, host clock around a drained stream (allocations, the download of
                           the ten loss values and the Python between the calls included); trainer_update_half_wall_ms: the two
                           device calls of the update alone, the same clock
  host path                the update half without the two device calls: IrnGrads.to_state_dict() (one download of the gradient),
                           the float32 update in numpy on every parameter, load_state_dict and the re-creation of the net and
                           of its wsc_irn_grad (the whole backbone is packed again: the net has no partial update) -- host clock
                           per part, and the step's wall time with that update half in place of the device's

One GPU step; run it under its own time limit:   timeout -k 10 420 python profiles/irn_train_step.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from oracle import irn_ref  # noqa: E402
from tests import irn_loss_ref  # noqa: E402
from tests import irn_sgd_ref as ref  # noqa: E402
from wsscam import _lib, irn_train  # noqa: E402
from wsscam.misc.indexing import PathIndex  # noqa: E402
from wsscam.net import resnet50_irn  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

N, S, REPS, HOST_REPS = 16, 512, 5, 2
LR, WD, MAX_STEP = 0.1, 1e-4, 1000

sd = {k: v.numpy() for k, v in irn_ref.make_resnet50_irn_state_dict(seed=3).items()}
m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=S, stride=4, precision=_lib.PREC_F16X3)
m.load_state_dict(sd)
m.eval().cuda(0)
ctx, net = m.ctx, m._ensure_net()
path_index = PathIndex(10)
rng = np.random.default_rng(N)
x = rng.normal(0, 1, (N, 3, S, S)).astype(np.float32)
label = irn_loss_ref.block_labels(rng, N, S // 4, S // 4)


def timed(fn, reps):
    fn()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return ctx.timer_end() / reps


def wall(fn, reps):
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


out = {"N": N, "S": S, "precision": "f16x3"}
with irn_train.IrnTrainer(m, path_index, LR, WD, MAX_STEP) as tr, DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, label) as ld:
    grad = tr.grad
    entries, elems = net.edge_tape_plan(N, S)
    (He, We), (Hd, Wd) = net.edge_size(S)
    dirs, start, yx = tr.loss.tables
    with DeviceMaps(ctx, (elems,), np.float32) as tape, DeviceMaps(ctx, (N, He, We), np.float32) as edge, DeviceMaps(ctx, (N, 2, Hd, Wd), np.float32) as dp, \
            DeviceMaps(ctx, (N, He, We), np.float32) as de, DeviceMaps(ctx, (N, 2, Hd, Wd), np.float32) as dd, \
            DeviceMaps(ctx, (len(_lib.IRN_LOSS_SLOTS),), np.float64) as lo, DeviceMaps(ctx, (grad.grad_elems,), np.float32) as g, \
            DeviceMaps.from_host(ctx, tr.params.to_host()) as p2, DeviceMaps.from_host(ctx, tr.mom.to_host()) as m2:
        out["forward_edge_tape_ms"] = round(timed(lambda: net.forward_edge_tape(xd.ptr, N, S, tape.ptr, elems, edge.ptr, dp.ptr), REPS), 3)
        out["irn_aff_loss_ms"] = round(timed(lambda: _lib.irn_aff_loss(ctx, edge.ptr, dp.ptr, ld.ptr, N, He, We, dirs, start, yx, tr.loss.radius_floor,
                                                                       tr.loss.valid_below, lo.ptr, grad_edge_dev=de.ptr, grad_dp_dev=dd.ptr), REPS), 3)
        out["backward_edge_ms"] = round(timed(lambda: grad.backward(N, S, tape.ptr, elems, de.ptr, dd.ptr, g.ptr), REPS), 3)
        # (the update on a copy of the parameters: the trainer's own stay what the net holds)
        out["irn_sgd_step_ms"] = round(timed(lambda: grad.sgd_step(p2.ptr, g.ptr, m2.ptr, LR, 10 * LR, WD, WD), 200), 4)
        out["irn_load_params_ms"] = round(timed(lambda: grad.load_params(tr.params.ptr), 200), 4)
        out["trainer_update_half_wall_ms"] = round(wall(lambda: (grad.sgd_step(p2.ptr, g.ptr, m2.ptr, LR, 10 * LR, WD, WD),
                                                                 grad.load_params(tr.params.ptr)), REPS), 3)
    out["grad_floats"] = grad.grad_elems
    out["device_parts_sum_ms"] = round(sum(out[k] for k in ("forward_edge_tape_ms", "irn_aff_loss_ms", "backward_edge_ms", "irn_sgd_step_ms",
                                                            "irn_load_params_ms")), 3)
    out["trainer_step_wall_ms"] = round(wall(lambda: tr.step(xd, ld), REPS), 3)

# the host path: what a caller of the parent commit had to do with the gradient
loss = irn_train.AffinityLoss(path_index, ctx=ctx)
arch = "resnet50"
b = ref.boundary(sd, arch)
cur = dict(sd)
p, mom = ref.flat_params(cur, arch), np.zeros(ref.layout(cur, arch)[1], np.float32)
parts = {"grad_step": 0.0, "to_state_dict": 0.0, "numpy_update": 0.0, "load_state_dict_and_net": 0.0}
with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps.from_host(ctx, label) as ld:
    for rep in range(HOST_REPS + 1):
        t = [time.perf_counter()]
        losses, grads = loss.grad_step(m, xd, ld)
        ctx.sync()
        t.append(time.perf_counter())
        with grads:
            gsd = grads.to_state_dict()
        t.append(time.perf_counter())
        p, mom = ref.sgd_step32(p, ref.flat_params(gsd, arch), mom, b, LR, 10 * LR, WD, WD)
        cur.update(ref.unflatten(p, cur, arch))
        t.append(time.perf_counter())
        m.load_state_dict(cur)
        m.cuda(0)
        m.irn_grad()
        ctx.sync()
        t.append(time.perf_counter())
        if rep:  # (the first round is the warm-up)
            for k, (a, c) in zip(parts, zip(t[:-1], t[1:])):
                parts[k] += (c - a) * 1e3 / HOST_REPS
out["host_path_ms"] = {k: round(v, 2) for k, v in parts.items()}
out["host_path_step_wall_ms"] = round(sum(parts.values()), 2)
out["host_path_update_half_ms"] = round(sum(v for k, v in parts.items() if k != "grad_step"), 2)
m._release_net()
print(json.dumps(out))
