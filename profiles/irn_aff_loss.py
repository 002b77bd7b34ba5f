"""The IRNet training loss at the reference's size: crop 512 -> 128 x 128 maps, PathIndex(radius=10) (step/train_irn.py:16):
152 directions, 2134 path pixels, 13 090 sources, 1 989 680 pairs per image; B = 16 and 32; 4 x 4 label blocks of which a third
is `ignore`, so that about half of the pairs are valid (the share is printed).

Prints one JSON line per batch size: kernel time of wsc_irn_aff_loss (device events, buffers resident) without a gradient and
with both; wall time of irn_train.AffinityLoss on device maps (call + download of the ten values); the bytes the call moves
(computed from the shapes: the staged tiles with their halos, the integer planes zeroed, added to and read, the gradients);
and, on the same card, the reference's formulation in float32 torch (torch_step below, restated here: index_select per path
length, max_pool2d, the four loss tensors, the reductions, backward()), forward + backward, with the floats it materialises.

One GPU step; run it under its own time limit:   timeout -k 10 300 python profiles/irn_aff_loss.py"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wsss-analysis_amd")]
from tests import irn_loss_ref as ref  # noqa: E402
from wsscam import _lib, irn_train  # noqa: E402
from wsscam.misc.indexing import PathIndex  # noqa: E402
from wsscam.secdsrg import DeviceMaps  # noqa: E402

H = W = 128
RADIUS, REPS, TORCH_REPS = 10, 50, 5
LABEL_VALUES = np.array([0, 0, 3, 7, 255, 255], np.uint8)


def torch_step(e, d, bg, fg, neg, path_idx, dst, rf):
    """AffinityDisplacementLoss.forward + the reductions of the training step + backward, float32 on the device"""
    e = e.detach().requires_grad_(True)
    d = d.detach().requires_grad_(True)
    B, h, w = e.shape
    x = torch.sigmoid(e).view(B, -1)
    affs = []
    for ind in path_idx:
        dist = torch.index_select(x, 1, ind.view(-1)).view(B, *ind.shape)
        affs.append(1 - F.max_pool2d(dist, (ind.shape[1], 1)).squeeze(2))
    aff = torch.cat(affs, dim=1)
    pos_term, neg_term = -torch.log(aff + 1e-5), -torch.log(1. + 1e-5 - aff)
    ch, cw = h - rf, w - 2 * rf
    src = d[:, :, :ch, rf:rf + cw]
    pair = (src.unsqueeze(2) - torch.stack([d[:, :, dy:dy + ch, rf + dx:rf + dx + cw] for dy, dx in dst], 2)).reshape(B, 2, len(dst), -1)
    target = torch.tensor(dst, dtype=torch.float32, device=e.device).t().reshape(1, 2, -1, 1)
    fg_dp, bg_dp = torch.abs(pair - target), torch.abs(pair)
    pos = (bg * pos_term).sum() / (bg.sum() + 1e-5) / 2 + (fg * pos_term).sum() / (fg.sum() + 1e-5) / 2
    ng = (neg * neg_term).sum() / (neg.sum() + 1e-5)
    dp_fg = (fg_dp * fg.unsqueeze(1)).sum() / (2 * fg.sum() + 1e-5)
    dp_bg = (bg_dp * bg.unsqueeze(1)).sum() / (2 * bg.sum() + 1e-5)
    total = (pos + ng) / 2 + (dp_fg + dp_bg) / 2
    total.backward()
    return total.detach(), e.grad, d.grad


ctx = _lib.Context(0)
pi = PathIndex(RADIUS, default_size=(H, W))
rf = pi.radius_floor
dirs, start, yx = pi.device_tables()
D, S = len(dirs), len(pi.src_indices)
TX, TY = 32, 8  # the tile of csrc/irn_loss.hip
tiles = -(-(W - 2 * rf) // TX) * -(-(H - rf) // TY)
dev = torch.device("cuda:0")
path_idx = [torch.from_numpy(p).to(dev) for p in pi.path_indices]
dst = [tuple(int(v) for v in p) for p in pi.search_dst]

for B in (16, 32):
    rng = np.random.default_rng(B)
    edge = (2.0 * rng.standard_normal((B, H, W))).astype(np.float32)
    dp = (3.0 * rng.standard_normal((B, 2, H, W))).astype(np.float32)
    label = ref.block_labels(rng, B, H, W, values=LABEL_VALUES)
    bg, fg, neg = ref.pair_labels(label, pi)
    valid_share = float((bg.sum() + fg.sum() + neg.sum()) / bg.size)
    e_dev, d_dev, l_dev = (DeviceMaps.from_host(ctx, a) for a in (edge, dp, label))
    loss_dev = DeviceMaps(ctx, (len(_lib.IRN_LOSS_SLOTS),), np.float64)
    ge_dev, gd_dev = DeviceMaps(ctx, edge.shape, np.float32), DeviceMaps(ctx, dp.shape, np.float32)

    def call(ge=None, gd=None):
        _lib.irn_aff_loss(ctx, e_dev.ptr, d_dev.ptr, l_dev.ptr, B, H, W, dirs, start, yx, rf, 21, loss_dev.ptr, grad_edge_dev=ge, grad_dp_dev=gd)

    kernel_ms = {}
    for name, kw in (("loss_only", {}), ("with_both_grads", {"ge": ge_dev.ptr, "gd": gd_dev.ptr})):
        for _ in range(5):
            call(**kw)
        ctx.timer_begin()
        for _ in range(REPS):
            call(**kw)
        kernel_ms[name] = round(ctx.timer_end() / REPS, 4)
    total_dev = float(loss_dev.to_host()[6])
    ge_host = ge_dev.to_host()

    al = irn_train.AffinityLoss(pi, ctx=ctx)

    def step():
        losses, g_e, g_d = al(e_dev, d_dev, l_dev)
        g_e.free()
        g_d.free()
        return losses

    for _ in range(5):
        step()
    t0 = time.perf_counter()
    for _ in range(REPS):
        step()
    wall_ms = (time.perf_counter() - t0) / REPS * 1e3
    for m in (e_dev, d_dev, l_dev, loss_dev, ge_dev, gd_dev):
        m.free()

    te, td = torch.from_numpy(edge).to(dev), torch.from_numpy(dp).to(dev)
    tbg, tfg, tneg = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (bg, fg, neg))
    for _ in range(2):
        total_t, g_e, g_d = torch_step(te, td, tbg, tfg, tneg, path_idx, dst, rf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(TORCH_REPS):
        total_t, g_e, g_d = torch_step(te, td, tbg, tfg, tneg, path_idx, dst, rf)
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) / TORCH_REPS * 1e3
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    # float32 torch carries the losses to ~1e-6 and drops digits of 1 - sigmoid: a sanity check that both sides compute the same
    # thing, not a parity claim
    g_edge_diff = float(np.abs(g_e.cpu().numpy() - ge_host).max() / np.abs(ge_host).max())
    assert abs(float(total_t) - total_dev) <= 1e-3 * abs(total_dev) and g_edge_diff <= 1e-2, (float(total_t), total_dev, g_edge_diff)
    del te, td, tbg, tfg, tneg, g_e, g_d
    torch.cuda.empty_cache()

    planes = B * 7 * H * W * 4
    dev_bytes = B * tiles * (TX + 2 * rf) * (TY + rf) * 13 + 3 * planes + B * H * W * 4 * 4
    gathered = sum(int(p.size) for p in pi.path_indices)  # the index_select copies, floats per image
    ref_floats = B * (gathered + 2 * D * S + 2 * 2 * D * S + 3 * D * S)  # + pos / neg terms, the two dp loss tensors, the three label tensors
    print(json.dumps({"B": B, "shape": [H, W], "radius": RADIUS, "pairs_per_image": D * S, "valid_pair_share": round(valid_share, 3),
                      "kernel_ms_per_call": kernel_ms, "affinityloss_wall_ms_per_call": round(wall_ms, 4),
                      "device_bytes_per_call": dev_bytes, "launches_per_call": "4 + one memset (pair, reduce, pixel, reduce)",
                      "torch_f32_fwd_bwd_ms_per_call": round(torch_ms, 2), "torch_peak_allocated_GiB": round(peak_gb, 2),
                      "torch_forward_tensor_bytes": 4 * ref_floats, "total_device": total_dev, "total_torch_f32": float(total_t),
                      "g_edge_max_diff_vs_torch_f32_rel": g_edge_diff}))
