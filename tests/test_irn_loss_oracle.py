"""CPU: the float64 oracle of the IRNet training loss (tests/irn_loss_ref.py) against itself -- its two independent forms, the
reference's sigmoid-first order against the logits-first order the device uses, a pair worked by hand, and autograd against
central differences."""
import math

import numpy as np
import pytest

from tests import irn_loss_ref as ref

SMALL = [(2, 1, 2, 3), (3, 2, 9, 11), (5, 2, 16, 20)]


@pytest.mark.parametrize("case", SMALL, ids=str)
def test_tensor_form_equals_pair_loop(case):
    edge, dp, label = ref.make_case(case)
    a = ref.tensor_form(edge, dp, label, case[0], grad=False)["loss"]
    b = ref.pair_loop(edge, dp, label, case[0])
    for k in ref.KEYS:
        assert abs(a[k] - b[k]) <= 1e-12 * max(1.0, abs(b[k])), (k, a[k], b[k])
    if case[0] > 2:
        assert min(a["n_bg"], a["n_fg"], a["n_neg"]) > 0  # every term is live


@pytest.mark.parametrize("case", SMALL, ids=str)
def test_logits_first_equals_sigmoid_first(case):
    edge, dp, label = ref.make_case(case)
    a = ref.tensor_form(edge, dp, label, case[0])
    b = ref.tensor_form(edge, dp, label, case[0], sigmoid_first=True)
    assert a["tied"] == 0.0  # tie-free input: the two orders pick the same pixel
    for k in ref.KEYS:
        assert abs(a["loss"][k] - b["loss"][k]) <= 1e-12 * max(1.0, abs(b["loss"][k])), k
    for g in ("g_edge", "g_dp"):
        assert np.abs(a[g] - b[g]).max() <= 1e-12 * max(1.0, np.abs(b[g]).max()), g


def test_one_pair_by_hand():
    """radius 2 on a 2 x 3 map: one source, (0, 1), and four directions; the labels leave the pair to (0, 2) alone, a background
    pair whose path is its two end points."""
    edge = np.array([[[0.5, -0.25, 1.5], [2.0, 3.0, -1.0]]], np.float32)
    dp = np.array([[[[0.0, 0.75, -0.5], [0.0, 0.0, 0.0]], [[0.0, -1.0, -1.0], [0.0, 0.0, 0.0]]]], np.float32)
    label = np.array([[[255, 0, 0], [255, 255, 255]]], np.uint8)
    out = ref.tensor_form(edge, dp, label, 2)
    loss = out["loss"]
    assert (loss["n_bg"], loss["n_fg"], loss["n_neg"]) == (1.0, 0.0, 0.0)
    sig = 1.0 / (1.0 + math.exp(-1.5))  # the maximum of the path (0, 2), (0, 1) is 1.5, at the destination
    aff = 1.0 - sig
    pos_bg = -math.log(aff + 1e-5) / (1 + 1e-5)
    dp_bg = (abs(0.75 - -0.5) + abs(-1.0 - -1.0)) / (2 + 1e-5)
    want = {"pos_bg": pos_bg, "pos_fg": 0.0, "pos": pos_bg / 2, "neg": 0.0, "dp_fg": 0.0, "dp_bg": dp_bg,
            "total": pos_bg / 4 + dp_bg / 2}
    for k, v in want.items():
        assert loss[k] == pytest.approx(v, rel=1e-14, abs=1e-300), k
    g_edge = np.zeros((1, 2, 3))
    g_edge[0, 0, 2] = 0.25 / (1 + 1e-5) * aff * sig / (aff + 1e-5)
    g_dp = np.zeros((1, 2, 2, 3))
    g_dp[0, 0, 0, 1], g_dp[0, 0, 0, 2] = 0.5 / (2 + 1e-5), -0.5 / (2 + 1e-5)  # channel 1: pd == 0, no gradient
    assert np.abs(out["g_edge"] - g_edge).max() <= 1e-15 and np.abs(out["g_dp"] - g_dp).max() <= 1e-15
    assert ref.pair_loop(edge, dp, label, 2)["total"] == pytest.approx(want["total"], rel=1e-14)


def test_all_ignore_is_all_zero():
    edge, dp, _ = ref.make_case((3, 2, 9, 11))
    out = ref.tensor_form(edge, dp, np.full((2, 9, 11), 255, np.uint8), 3)
    assert all(v == 0.0 for v in out["loss"].values())
    assert not out["g_edge"].any() and not out["g_dp"].any()
    assert all(v == 0.0 for v in ref.pair_loop(edge, dp, np.full((2, 9, 11), 255, np.uint8), 3).values())


def test_autograd_equals_central_differences():
    case = (3, 1, 6, 7)
    edge, dp, _ = ref.make_case(case)
    label = ref.block_labels(np.random.default_rng(5), 1, 6, 7, values=np.array([0, 0, 3, 7], np.uint8), block=2)
    out = ref.tensor_form(edge, dp, label, 3)
    assert min(out["loss"][k] for k in ("n_bg", "n_fg", "n_neg")) > 0
    eps = 1e-6  # far below the gaps between path maxima and between pd and its kinks on this input
    e64, d64 = edge.astype(np.float64), dp.astype(np.float64)

    def total(e, d):
        return ref.tensor_form(e, d, label, 3, grad=False)["loss"]["total"]

    for name, arr, g in (("edge", e64, out["g_edge"]), ("dp", d64, out["g_dp"])):
        for idx in np.ndindex(arr.shape):
            hi, lo = arr.copy(), arr.copy()
            hi[idx] += eps
            lo[idx] -= eps
            fd = (total(hi, d64) - total(lo, d64)) / (2 * eps) if name == "edge" else (total(e64, hi) - total(e64, lo)) / (2 * eps)
            assert abs(fd - g[idx]) <= 1e-7 * max(1.0, np.abs(g).max()), (name, idx, fd, g[idx])
