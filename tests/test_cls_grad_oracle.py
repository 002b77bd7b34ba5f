"""CPU: the oracle of the 01_train backward pass (tests/cls_grad_ref.py) against torch itself.

  chain_grads on a float64 tape IS whole-graph autograd (the definition "the chain rule evaluated at the tape" loses nothing when the
  tape is exact), for both stacks, with and without BatchNorm, torch's and Keras' pools;
  the BatchNorm rule is torch.nn.BatchNorm2d's in train mode, running statistics included, under keep = 1 - momentum;
  the pool gradient's tie rule on hand-made windows;
  R32_CHAIN_CLS, the float32 evaluation's own error on one float32 tape, is re-measured and held to 1.5 x its recorded value."""
import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import cls_grad_ref as gref

# thin twins of the stacks for the identities (the widths do not matter to them): (root, batchnorm, pools, (H, W))
THIN = {"vgg16": [("layer1", [8, 8, "M"]), ("layer2", [8, 8, "M"]), ("layer3", [8, 8, 8, "M"]), ("layer4", [8, 8, 8, 8, 8, 8]),
                  ("layer5", [16, "D", 16, "D"])],
        "m7": [("layer1", [8, 8, "M"]), ("layer2", [8, 8, "M"]), ("layer3_p1", [8, 8, 8])]}
THIN_CASES = [("vgg16", True, None, (33, 33)), ("vgg16", False, gref.KERAS_POOLS, (40, 24)), ("m7", True, gref.KERAS_POOLS, (17, 21)),
              ("m7", True, [(2, 2, "valid"), (3, 1, "same"), (2, 2, "valid")], (18, 15)), ("m7", False, None, (12, 12))]


@pytest.fixture
def thin(monkeypatch):
    monkeypatch.setattr(gref, "CFG", THIN)


@pytest.mark.parametrize("case", THIN_CASES, ids=gref.case_id)
def test_chain_on_a_float64_tape_is_autograd(thin, case):
    root, bn, pools, hw = case
    sd = cnn_ref.make_plain_state_dict(root, THIN[root], 5, bn, seed=3)
    x = gref.net_input(hw)
    tape, feat = gref.forward_tape(root, sd, x, pools)
    assert ("%s.layer1.0.bn" % root in tape) == bn and "pool:1" in tape
    dfeat = np.random.default_rng(5).standard_normal(feat.shape)
    want = gref.autograd_grads(root, sd, x, dfeat, pools)
    got = gref.chain_grads(root, sd, tape, dfeat, pools)
    assert list(got) and sorted(got) == sorted(want) == sorted(gref.param_names(root, sd))
    worst = gref.worst_ratio(got, want)
    print("chain vs autograd %s: worst max|d| / max|g| %.3e at %s" % ((gref.case_id(case),) + worst))
    assert worst[0] <= 1e-12
    for n, w in want.items():
        assert np.abs(w).max() > 0, n


@pytest.mark.parametrize("momentum", [0.01, 0.1, 1.0])
def test_batch_norm_rule_is_torch_train_mode(momentum):
    """forward, the three gradients and the running statistics of nn.BatchNorm2d(eps = 1e-3) in train mode; torch's momentum weighs
    the NEW value, `keep` the old one: keep = 1 - momentum, and torch's running variance is the unbiased one"""
    rng = np.random.default_rng(2)
    N, C, H, W = 3, 6, 5, 4
    a = torch.from_numpy(rng.standard_normal((N, C, H, W)) * 3 + 1).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C, eps=gref.EPS, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C)))
        bn.bias.copy_(torch.from_numpy(rng.standard_normal(C)))
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(C)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, C)))
    run0 = (bn.running_mean.clone(), bn.running_var.clone())
    dy = torch.from_numpy(rng.standard_normal((N, C, H, W)))
    y = bn(a)
    y.backward(dy)
    mean, rstd = gref.bn_stats_t(a.detach())
    M = N * H * W
    a2 = a.detach().permute(0, 2, 3, 1).reshape(M, C).numpy()
    m64, v64, r64, y64 = gref.bn_train_ref(a2, bn.weight.detach().numpy(), bn.bias.detach().numpy())
    assert np.allclose(y.detach().permute(0, 2, 3, 1).reshape(M, C).numpy(), y64, rtol=1e-12, atol=1e-12)
    assert np.allclose(mean.numpy(), m64, rtol=1e-13) and np.allclose(rstd.numpy(), r64, rtol=1e-13)
    da, dgamma, dbeta = gref.bn_grad_t(a.detach(), mean, rstd, bn.weight.detach(), dy)
    for got, want in ((da, a.grad), (dgamma, bn.weight.grad), (dbeta, bn.bias.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12)
    keep = 1.0 - momentum
    assert np.allclose(bn.running_mean.numpy(), keep * run0[0].numpy() + (1 - keep) * m64, rtol=1e-13)
    assert np.allclose(bn.running_var.numpy(), keep * run0[1].numpy() + (1 - keep) * v64 * M / (M - 1), rtol=1e-13)


def test_pool_gradient_tie_rule_on_hand_made_windows():
    """a window's dy goes to its first maximum in row-major window order; padding is never a candidate; overlapping windows add"""
    x = np.zeros((1, 4, 4, 1))
    dy = np.arange(1, 5, dtype=np.float64).reshape(1, 2, 2, 1)
    dx = gref.pool_grad_ref(x, dy, ("torch", 2, 2, 0))[0, :, :, 0]  # all-zero windows: the top-left tap of each
    assert np.array_equal(dx, [[1, 0, 2, 0], [0, 0, 0, 0], [3, 0, 4, 0], [0, 0, 0, 0]])
    x[0, :, :, 0] = [[1, 5, 5, 0], [5, 2, 0, 0], [0, 0, 7, 7], [0, 0, 7, 7]]
    dx = gref.pool_grad_ref(x, dy, ("torch", 2, 2, 0))[0, :, :, 0]  # repeated maxima: (0, 1) before (1, 0); (0, 2) alone; (2, 2) first of four
    assert np.array_equal(dx, [[0, 1, 2, 0], [0, 0, 0, 0], [3, 0, 4, 0], [0, 0, 0, 0]])
    # 3 x 3 / 2 SAME on 4 x 4: out 2 x 2, no padding before, one row / column behind; the windows overlap on row / column 2
    x[0, :, :, 0] = [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 9, 0], [0, 0, 0, 0]]
    dx = gref.pool_grad_ref(x, dy, ("tf", 3, 2, 1))[0, :, :, 0]
    assert np.array_equal(dx, [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 10, 0], [0, 0, 0, 0]])
    # negative values under SAME padding: the padding (-inf) does not win, the in-image maximum does
    x[0, :, :, 0] = -np.arange(1, 17).reshape(4, 4)
    dx = gref.pool_grad_ref(x, dy, ("tf", 3, 2, 1))[0, :, :, 0]
    assert np.array_equal(dx, [[1, 0, 2, 0], [0, 0, 0, 0], [3, 0, 4, 0], [0, 0, 0, 0]])
    # VALID 2 x 2 / 2 on 5 x 5: the last row and column belong to no window
    dx = gref.pool_grad_ref(np.ones((1, 5, 5, 1)), dy, ("tf", 2, 2, 0))[0, :, :, 0]
    assert not dx[4].any() and not dx[:, 4].any() and dx.sum() == 10


def test_float32_chain_error():
    """R32_CHAIN_CLS: chain_grads in float32 against float64 on one float32 tape, over the GPU cases"""
    worst = (0.0, "", "")
    for case in gref.GRAD_CASES:
        root, bn, pools, hw = case
        sd = gref.state_dict(root, bn)
        tape32, feat = gref.forward_tape(root, sd, gref.net_input(hw), pools, dtype=torch.float32)
        dfeat = gref.case_dfeat(case, feat.shape)
        g64 = gref.chain_grads(root, sd, tape32, dfeat, pools, dtype=torch.float64)
        g32 = gref.chain_grads(root, sd, tape32, dfeat, pools, dtype=torch.float32)
        r = gref.worst_ratio(g32, g64)
        print("float32 chain %s: worst max|g32 - g64| / max|g64| %.3e at %s" % ((gref.case_id(case),) + r))
        worst = max(worst, r + (gref.case_id(case),))
    print("R32_CHAIN_CLS measured %.3e (%s of %s), recorded %.3e" % (worst + (gref.R32_CHAIN_CLS,)))
    assert 0 < worst[0] <= 1.5 * gref.R32_CHAIN_CLS
