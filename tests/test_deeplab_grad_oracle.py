"""CPU: the oracle of the DeepLab backward pass (tests/deeplab_grad_ref.py) against plain autograd and hand-checkable facts, and
the measurements behind R32_CHAIN (thin nets) and R32_CHAIN_FULL (the real widths, FULL_GRAD_CASES)."""
import functools

import numpy as np
import pytest
import torch

from tests import deeplab_grad_ref as gref
from tests import deeplab_ref as ref


def _case_id(case):
    return "%s-%d-%dx%d" % (case[0], case[1], case[2][0], case[2][1]) + ("-B%d-full" % case[3] if len(case) == 4 else "")


def case_inputs(case):
    """-> (weights, x): thin_case's (B = 2) for the THIN_CASES, the same recipe at 97 x 97; full_case's for a FULL_GRAD_CASES entry"""
    if len(case) == 4:
        return gref.full_case(case)
    method, C, hw = case
    weights, x = ref.thin_case(method, C, hw)
    return weights, x


def dfc8_for(case, shape):
    if len(case) == 4:
        return gref.full_dfc8(case, shape)
    method, C, hw = case
    rng = np.random.default_rng(900 + 3 * C + hw[1] + (1 if method == "SEC" else 0))
    return (1e-3 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("case", gref.GRAD_CASES + gref.FULL_GRAD_CASES, ids=_case_id)
def test_chain_on_float64_tape_is_autograd(case):
    """With a float64 tape the chain rule evaluated at the tape IS whole-graph autograd: <= 1e-12 of each layer's max|g|."""
    method = case[0]
    weights, x = case_inputs(case)
    tape, fc8 = gref.forward_tape(method, weights, x, torch.float64)
    dfc8 = dfc8_for(case, fc8.shape)
    chain = gref.chain_grads(method, weights, tape, dfc8, torch.float64)
    auto = gref.autograd_grads(method, weights, x, dfc8, torch.float64)
    assert set(chain) == set(ref.layer_names(method))
    ratios = gref.layer_ratio(chain, auto)
    print("chain on a float64 tape vs autograd, %s: worst %.2e" % (_case_id(case), max(max(r) for r in ratios.values())))
    for layer, (rw, rb) in ratios.items():
        assert rw <= 1e-12 and rb <= 1e-12, (layer, rw, rb)


@functools.lru_cache(maxsize=None)
def _float32_chain_error(case):
    method = case[0]
    weights, x = case_inputs(case)
    tape, fc8 = gref.forward_tape(method, weights, x, torch.float32)
    dfc8 = dfc8_for(case, fc8.shape)
    g32 = gref.chain_grads(method, weights, tape, dfc8, torch.float32)
    g64 = gref.chain_grads(method, weights, tape, dfc8, torch.float64)
    ratios = gref.layer_ratio(g32, g64)
    layer = max(ratios, key=lambda l: max(ratios[l]))
    return max(ratios[layer]), layer


def test_float32_chain_error():
    """R32_CHAIN: the float32 chain against the float64 chain on one float32 tape, worst layer over the ten cases."""
    worst = max((_float32_chain_error(case) + (case,) for case in gref.GRAD_CASES), key=lambda t: t[0])
    print("float32 chain vs float64 chain on one float32 tape: worst %.3e at %s of %s; R32_CHAIN = %.3e" % (worst + (gref.R32_CHAIN,)))
    assert worst[0] <= 1.5 * gref.R32_CHAIN


def test_float32_chain_error_full_width():
    """R32_CHAIN_FULL: the same measurement at the real widths (fc 1024, 21 classes), worst layer over FULL_GRAD_CASES."""
    worst = max((_float32_chain_error(case) + (_case_id(case),) for case in gref.FULL_GRAD_CASES), key=lambda t: t[0])
    print("float32 chain vs float64 chain on one float32 tape, full width: worst %.3e at %s of %s; R32_CHAIN_FULL = %.3e"
          % (worst + (gref.R32_CHAIN_FULL,)))
    assert worst[0] <= 1.5 * gref.R32_CHAIN_FULL


def test_full_width_cases_are_not_vacuous_and_have_the_tap_patterns():
    """What the device test of FULL_GRAD_CASES relies on, stated on the oracle: every layer's gradient is non-zero, and fc6's
    live taps are the ones the map size leaves in the image."""
    centre = [[False, False, False], [False, True, False], [False, False, False]]
    column = [[False, True, False]] * 3
    for case in gref.FULL_GRAD_CASES:
        method, _, hw, _ = case
        weights, x = case_inputs(case)
        tape, fc8 = gref.forward_tape(method, weights, x, torch.float32)
        g64 = gref.chain_grads(method, weights, tape, dfc8_for(case, fc8.shape), torch.float64)
        smallest = min(min(np.abs(g["w"]).max(), np.abs(g["b"]).max()) for g in g64.values())
        print("%s: smallest max|g64| over the layers %.3e" % (_case_id(case), smallest))
        assert smallest > 0
        for sfx, _ in gref.branches(method):
            w6 = g64["fc6" + sfx]["w"]
            live = [[bool(w6[r, s].any()) for s in range(3)] for r in range(3)]
            want = centre if sfx != "_1" else ([[True] * 3] * 3 if hw == (65, 65) else column)
            assert live == want, (case, sfx, live)
            assert not np.signbit(w6[~np.array(live)]).any()


def test_pointwise_conv_wgrad_is_xt_dz():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 4, 3, 5)).astype(np.float32)
    dz = rng.standard_normal((2, 4, 3, 7)).astype(np.float32)
    dw, db, S, n, Sb = gref.wgrad_ref(x, dz, 1, 1)
    X, Z = x.reshape(-1, 5).astype(np.float64), dz.reshape(-1, 7).astype(np.float64)
    np.testing.assert_allclose(dw[0, 0], X.T @ Z, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(db, Z.sum(0), rtol=1e-13)
    np.testing.assert_allclose(S[0, 0], np.abs(X).T @ np.abs(Z), rtol=1e-13)
    assert n.tolist() == [[24.0]]


def test_centre_tap_only_layer_has_eight_zero_taps():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 9, 9, 4)).astype(np.float32)
    dz = rng.standard_normal((1, 9, 9, 3)).astype(np.float32)
    dw, _, _, n, _ = gref.wgrad_ref(x, dz, 3, 12)
    assert n.tolist() == [[0, 0, 0], [0, 81, 0], [0, 0, 0]]
    assert np.count_nonzero(dw[1, 1]) == 12
    dw[1, 1] = 0
    assert not dw.any()


def test_all_equal_window_sends_gradient_to_first_element():
    x = np.full((1, 3, 3, 1), 0.25, np.float32)
    dy = np.zeros((1, 3, 3, 1), np.float32)
    dy[0, 1, 1, 0] = 1.0  # the centre window: the whole map
    dx, _ = gref.pool_grad_ref(x, dy, False, 1)
    want = np.zeros((3, 3))
    want[0, 0] = 1.0
    assert dx[0, :, :, 0].tolist() == want.tolist()


def test_pool5a_corner_divides_by_four():
    x = np.zeros((1, 5, 5, 1), np.float32)
    dy = np.zeros((1, 5, 5, 1), np.float32)
    dy[0, 0, 0, 0] = 1.0
    dx, _ = gref.pool_grad_ref(x, dy, True, 1)
    want = np.zeros((5, 5))
    want[:2, :2] = 0.25
    assert dx[0, :, :, 0].tolist() == want.tolist()
