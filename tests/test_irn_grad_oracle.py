"""CPU: the oracle of the IRNet heads' backward pass (tests/irn_grad_ref.py) against torch.double autograd, the float64 forms of the
two per-op kernels against autograd of the torch ops, a directional derivative of the whole loss -> heads chain, the measurements
behind R32_GN and R32_IRN_CHAIN, and the exports the pass adds."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import irn_ref
from tests import irn_grad_ref as gref
from tests import irn_loss_ref

CASES = [("resnet50", 64), ("resnet50", 68), ("vgg16", 64), ("m7", 64)]


@functools.lru_cache(maxsize=None)
def state_dict(arch):
    return {"resnet50": irn_ref.make_resnet50_irn_state_dict, "vgg16": irn_ref.make_vgg16_irn_state_dict,
            "m7": irn_ref.make_m7_irn_state_dict}[arch](seed=3)


@functools.lru_cache(maxsize=None)
def forward(arch, S, N=2):
    """-> (x, tape, edge, dp) of a float64 host pass, shared and never modified"""
    x = np.random.default_rng(10 + S).normal(0, 1, (N, 3, S, S)).astype(np.float32)
    return (x,) + gref.host_tape(x, state_dict(arch), arch)


def head_gradients(shape_e, shape_d, seed):
    rng = np.random.default_rng(seed)
    return (1e-3 * rng.standard_normal(shape_e)).astype(np.float32), (1e-3 * rng.standard_normal(shape_d)).astype(np.float32)


@pytest.mark.parametrize("arch,S", CASES)
def test_manual_backward_is_autograd(arch, S):
    sd = state_dict(arch)
    x, tape, edge, dp = forward(arch, S)
    if (arch, S) == ("resnet50", 68):  # every crop of the net is non-trivial here
        assert [tape["x%d" % k].shape[1] for k in range(1, 6)] == [17, 17, 9, 5, 5]
    d_edge, d_dp = head_gradients(edge.shape, dp.shape, 20 + S)
    names = sum(gref.param_names(arch), [])
    sd64 = {k: v.double() for k, v in sd.items()}
    for n in names:
        sd64[n] = sd64[n].clone().requires_grad_(True)
    e, d = irn_ref.irn_net_forward(torch.from_numpy(x).double(), sd64, arch)
    # the host tape is that forward pass (dp_out: MeanShift, a constant, subtracted by the restatement)
    assert np.abs(e.detach().numpy()[:, 0] - edge).max() <= 1e-10 * np.abs(edge).max()
    assert np.abs((d + sd64["mean_shift.running_mean"].view(1, 2, 1, 1)).detach().numpy() - dp).max() <= 1e-10 * np.abs(dp).max()
    ((e[:, 0] * torch.from_numpy(d_edge).double()).sum() + (d * torch.from_numpy(d_dp).double()).sum()).backward()
    want = {n: sd64[n].grad.numpy() for n in names}
    got = gref.head_grads(tape, sd, arch, d_edge, d_dp)
    assert set(got) == set(names) and all(got[n].shape == tuple(sd[n].shape) for n in names)
    worst = gref.worst_ratio(got, want)
    print("manual backward vs torch.double autograd, %s S = %d: worst max|d| / max|g| %.2e at %s" % ((arch, S) + worst))
    assert min(np.abs(g).max() for g in want.values()) > 0
    for n in names:
        assert np.abs(got[n] - want[n]).max() <= 1e-10 * np.abs(want[n]).max(), n


@pytest.mark.parametrize("case", [(2, 9, 9, 32, 2, 17, 17, 192, 64), (1, 5, 5, 32, 4, 17, 17, 192, 128), (1, 1, 1, 32, 4, 3, 2, 192, 96),
                                  (1, 1, 7, 64, 2, 2, 14, 448, 0), (3, 6, 4, 64, 1, 6, 4, 448, 0), (2, 8, 8, 256, 2, 16, 16, 448, 192)])
def test_upsample_adjoint_is_autograd(case):
    N, H, W, C, up, Hd, Wd, Ctot, coff = case
    rng = np.random.default_rng(sum(case))
    y = rng.standard_normal((N, H, W, C))
    dcat = rng.standard_normal((N, Hd, Wd, Ctot))
    yt = torch.from_numpy(y).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    v = F.interpolate(yt, scale_factor=up, mode="bilinear", align_corners=False) if up != 1 else yt
    v = F.relu(v[..., :Hd, :Wd])
    cat = np.zeros((N, Hd, Wd, Ctot))
    cat[..., coff:coff + C] = v.detach().permute(0, 2, 3, 1).numpy()
    v.backward(torch.from_numpy(dcat[..., coff:coff + C]).permute(0, 3, 1, 2))
    want = yt.grad.permute(0, 2, 3, 1).numpy()
    got, mag, terms = gref.up_relu_grad(dcat, cat, H, W, C, up, coff)
    assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert terms.max() <= (2 * up) ** 2 and (mag >= np.abs(got) - 1e-12).all()


@pytest.mark.parametrize("case", gref.GN_CASES + [gref.GN_CONSTANT_CASE])
def test_group_norm_backward_is_autograd(case):
    constant = case == gref.GN_CONSTANT_CASE
    z, dy, gamma = gref.gn_case(case, 5, constant=constant)
    want = gref.torch_gn_grads(z, dy, gamma, case[4], torch.float64)
    got = gref.group_norm_grad(z, dy, gamma, case[4])
    for g, w in zip(got, want):
        assert np.isfinite(g).all()
        assert np.abs(g - w).max() <= 1e-10 * max(np.abs(w).max(), 1e-30)


def test_float32_group_norm_error():
    """R32_GN: torch float32 autograd against float64 on identical float32 operands, worst of GN_CASES per output.  (The
    constant-group case is left out of the figure: float32 autograd itself loses 7e-6 of dgamma there, rstd = 316 amplifying the
    rounding of its mean, and a bound built on that would be an order of magnitude wider for every case.)"""
    worst = {"dz": 0.0, "dgamma": 0.0, "dbeta": 0.0}
    for case in gref.GN_CASES:
        z, dy, gamma = gref.gn_case(case, 5)
        g32 = gref.torch_gn_grads(z, dy, gamma, case[4], torch.float32)
        g64 = gref.torch_gn_grads(z, dy, gamma, case[4], torch.float64)
        for key, a, b in zip(("dz", "dgamma", "dbeta"), g32, g64):
            worst[key] = max(worst[key], float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()))
    print("float32 vs float64 GroupNorm backward: %s; R32_GN = %s" % (worst, gref.R32_GN))
    for key in worst:
        assert worst[key] <= 1.5 * gref.R32_GN[key], key


def test_float32_chain_error():
    """R32_IRN_CHAIN: head_grads in float32 against float64 on one float32 tape"""
    arch, S = "resnet50", 64
    _, tape, edge, dp = forward(arch, S)
    tape32 = {k: v.astype(np.float32) for k, v in tape.items()}
    d_edge, d_dp = head_gradients(edge.shape, dp.shape, 7)
    sd = state_dict(arch)
    g64 = gref.head_grads(tape32, sd, arch, d_edge, d_dp, np.float64)
    g32 = gref.head_grads(tape32, sd, arch, d_edge, d_dp, np.float32)
    worst = gref.worst_ratio(g32, g64)
    print("float32 chain vs float64 chain on one float32 tape: worst %.3e at %s; R32_IRN_CHAIN = %.3e" % (worst + (gref.R32_IRN_CHAIN,)))
    assert worst[0] <= 1.5 * gref.R32_IRN_CHAIN


def test_directional_derivative_of_the_loss_through_the_heads():
    """d total / d t of total(theta + t v) by central differences against <head_grads(g_edge, g_dp), v>, everything float64"""
    arch, S, radius = "resnet50", 64, 5
    sd = state_dict(arch)
    x, tape, edge, dp = forward(arch, S)
    label = irn_loss_ref.block_labels(np.random.default_rng(4), 2, edge.shape[1], edge.shape[2])
    ref = irn_loss_ref.tensor_form(edge, dp, label, radius)
    assert min(ref["loss"][k] for k in ("n_bg", "n_fg", "n_neg")) > 0
    grads = gref.head_grads(tape, sd, arch, ref["g_edge"], ref["g_dp"])
    rng = np.random.default_rng(6)
    names = sum(gref.param_names(arch), [])
    v = {n: rng.standard_normal(tuple(sd[n].shape)) * float(sd[n].abs().max()) for n in names}
    slope = sum(float((grads[n] * v[n]).sum()) for n in names)
    table = gref.head_table(arch)
    xs = [tape["x%d" % k] for k in range(1, 6)]

    def total(t):
        moved = {k: (w.double().numpy() + t * v[k] if k in v else w) for k, w in sd.items()}
        _, e, d = gref._walk(xs, moved, arch, table, lambda kind, k, computed: computed)
        return irn_loss_ref.tensor_form(e, d, label, radius, grad=False)["loss"]["total"]

    # total is piecewise smooth: a step small enough that no ReLU or path maximum changes hands inside [-h, h] (1e-6 already
    # crosses some of the 5e5 ReLU inputs: its quotient is off by 6e-4) leaves O(h^2) truncation and 2^-53 |total| / h =
    # 2e-9 of rounding
    h = 1e-7
    fd = (total(h) - total(-h)) / (2 * h)
    print("directional derivative: central difference %.9e, chain %.9e, relative difference %.2e" % (fd, slope, abs(fd - slope) / abs(slope)))
    assert abs(fd - slope) <= 1e-6 * abs(slope) and abs(slope) > 0


def test_new_symbols_are_exported(built):
    from wsscam import _lib

    declared = _lib.check_exports()
    lib = _lib.load()
    for name in ("wsc_net_edge_tape_plan", "wsc_net_forward_edge_tape", "wsc_irn_grad_create", "wsc_irn_grad_destroy",
                 "wsc_irn_grad_layout", "wsc_net_backward_edge", "wsc_relu_upsample_grad_nhwc", "wsc_group_norm_grad_nhwc"):
        assert name in declared and hasattr(lib, name)
