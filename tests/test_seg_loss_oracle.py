"""CPU: the float64 oracle of the SEC / DSRG loss head (tests/seg_loss_ref.py) against autograd from the logits and against
hand-checkable facts; secdsrg.rank_weights; the header's export."""
import numpy as np
import pytest
import torch

from tests import seg_loss_ref as ref
from wsscam import _lib

M = float(np.float32(1e-4))


def _logit_case(shape, seed):
    """float64 logits whose sp-softmax has no ties, CRF log-probabilities, cues and labels as make_case draws them"""
    _, crf, cues, labels = ref.make_case(shape, seed)
    z = np.random.default_rng(seed).normal(0, 2, shape)
    return z, crf, cues, labels


@pytest.mark.parametrize("method", ["SEC", "DSRG"])
@pytest.mark.parametrize("shape", [(3, 7, 5, 5), (2, 9, 9, 32)], ids=lambda s: "x".join(map(str, s)))
def test_chain_rule_equals_autograd_from_the_logits(method, shape):
    """dL/dz by autograd with the float64 logits as the leaf == s (g_p - <g_p, s>) / (1 + C m) with g_p by autograd at p, and ==
    the same formula on the oracle's g_p (loss_1 / loss_3 placed by stable argsort): 1e-12 of the tensor's largest magnitude."""
    z_np, crf, cues, labels = _logit_case(shape, 3)
    z = torch.tensor(z_np, dtype=torch.float64, requires_grad=True)
    p = ref.sp_softmax(z, M)
    out, _ = ref.terms(method, p, ref.t64(crf), ref.t64(cues), ref.t64(labels))
    g_z_auto, g_p_auto = torch.autograd.grad(out["norm"], [z, p])
    g_z_auto, g_p_auto, p_np = g_z_auto.numpy(), g_p_auto.numpy(), p.detach().numpy()
    assert not ref.has_ties(p_np)
    scale = np.abs(g_z_auto).max()
    assert scale > 0
    assert np.abs(ref.grad_fc8(p_np, g_p_auto, M) - g_z_auto).max() <= 1e-12 * scale
    # the oracle's composite g_p: terms() on p as a float64 leaf, the rank terms placed by argsort
    p_leaf = torch.tensor(p_np, dtype=torch.float64, requires_grad=True)
    out2, _ = ref.terms(method, p_leaf, ref.t64(crf), ref.t64(cues), ref.t64(labels))
    names = ("seed", "constrain", "loss_2") if method == "SEC" else ("seed", "constrain")
    g_p = sum(torch.autograd.grad(out2[k], p_leaf, retain_graph=True)[0].numpy() for k in names)
    if method == "SEC":
        g1, g3 = ref.rank_term_grads(p_np, labels)
        g_p = g_p + g1 + g3
    assert np.abs(g_p - g_p_auto).max() <= 1e-12 * np.abs(g_p_auto).max()
    g_z = ref.grad_fc8(p_np, g_p, M)
    assert np.abs(g_z - g_z_auto).max() <= 1e-12 * scale
    # the softmax Jacobian annihilates constants: the classes' g_z sum to 0 at every pixel, within float64 rounding
    assert np.abs(g_z.sum(-1)).max() <= 64 * np.finfo(np.float64).eps * np.abs(g_z).sum(-1).max()


def test_evaluate_is_terms_plus_placed_rank_weights():
    prob, crf, cues, labels = ref.make_case((3, 7, 5, 5))
    losses, mag, g_p, g_z, parts = ref.evaluate("SEC", prob, crf, cues, labels)
    assert set(parts) == {"seed", "constrain", "loss_1", "loss_2", "loss_3"}
    assert losses["norm"] == pytest.approx(losses["seed"] + losses["expand"] + losses["constrain"], rel=1e-15)
    assert all(mag[k] >= abs(losses[k]) * (1 - 1e-12) for k in ref.KEYS)
    p = ref.t64(prob).requires_grad_(True)
    out, _ = ref.terms("SEC", p, ref.t64(crf), ref.t64(cues), ref.t64(labels))
    auto = torch.autograd.grad(out["norm"], p)[0].numpy()
    assert np.abs(g_p - auto).max() <= 1e-12 * np.abs(auto).max()  # no ties: autograd through the sort places the same weights
    losses_d, _, g_p_d, _, parts_d = ref.evaluate("DSRG", prob, crf, cues)
    assert set(parts_d) == {"seed", "constrain"} and losses_d["expand"] == 0.0
    assert losses_d["seed"] == pytest.approx(losses_d["seed_bg"] + losses_d["seed_fg"], rel=1e-15)


@pytest.mark.parametrize("n", [1, 35, 1681])
def test_rank_weights_are_the_references_expression(n):
    from wsscam import secdsrg

    for q in (0.996, 0.999):
        w, z = secdsrg.rank_weights(n, q)
        want = np.array([q ** i for i in range(n - 1, -1, -1)])
        assert w.dtype == np.float32 and w.shape == (n,) and isinstance(z, np.float32)
        assert np.array_equal(w, np.float32(want)) and z == np.float32(np.sum(want))
        assert w[-1] == 1.0
        w2, z2 = ref.rank_weights(n, q)
        assert np.array_equal(w, w2) and z == z2


def test_hand_checkable_facts():
    B, H, W, C = 2, 4, 3, 3
    prob, crf, cues, labels = ref.make_case((B, H, W, C))
    # a constant map has mean == value (up to the float32 rounding of the weights against their float32 sum)
    const = prob.copy()
    const[0, :, :, 1] = 0.25
    labels[:] = 1.0
    p = ref.t64(const)
    n = H * W
    w_fg, z_fg = ref.rank_weights(n, ref.Q_FG)
    mean = float((torch.sort(p.reshape(B, n, C)[0, :, 1])[0] * ref.t64(w_fg)).sum() / float(z_fg))
    assert mean == pytest.approx(0.25, rel=n * 2.0 ** -24)
    out, _ = ref.terms("SEC", p, ref.t64(crf), ref.t64(cues), ref.t64(labels))
    # ... so loss_1 of image 0 holds log(0.25) for that class
    alone = labels.copy()
    alone[:, 2] = 0.0
    out1, _ = ref.terms("SEC", p[:1], ref.t64(crf[:1]), ref.t64(cues[:1]), ref.t64(alone[:1]))
    assert float(out1["loss_1"]) == pytest.approx(-np.log(mean), rel=1e-14)
    # an image without cues contributes 0 to SEC's seed loss: image 1 of make_case has none
    assert cues[1].sum() == 0 and cues[0].sum() > 0
    one, _ = ref.terms("SEC", p[:1], ref.t64(crf[:1]), ref.t64(cues[:1]), ref.t64(labels[:1]))
    assert float(out["seed"]) == pytest.approx(0.5 * float(one["seed"]), rel=1e-15)
    # constrain == 0 for SEC when q == p
    same, _ = ref.terms("SEC", p, torch.log(p), ref.t64(cues), ref.t64(labels))
    assert abs(float(same["constrain"])) <= 1e-15
    # the maximum's share is split equally among tied maxima
    tied = prob.copy()
    tied[0, :, :, 1] = np.minimum(tied[0, :, :, 1], 0.5)
    tied[0, 0, 1, 1] = tied[0, 2, 2, 1] = tied[0, 3, 0, 1] = 0.75
    lab = np.zeros((B, C), np.float32)
    _, _, _, _, parts = ref.evaluate("SEC", tied, crf, cues, lab)
    g2 = parts["loss_2"][0, :, :, 1]
    share = (1.0 / B) / (C - 1) / (1 - 0.75) / 3
    assert np.count_nonzero(g2) == 3 and g2[0, 1] == pytest.approx(share, rel=1e-14) and g2[0, 1] == g2[2, 2] == g2[3, 0]
    # the rank weights of a tied group go out in pixel order
    g1, _ = ref.rank_term_grads(const, labels)
    assert (np.diff(g1[0, :, :, 1].reshape(-1)) < 0).all()  # every pixel ties: rank = pixel index, the weights grow with it


def test_make_case_has_the_issues_inputs():
    for shape in [(3, 7, 5, 5), (2, 41, 41, 21), (1, 1, 1, 2), (1, 128, 64, 2), (2, 9, 9, 32)]:
        prob, crf, cues, labels = ref.make_case(shape)
        assert prob.dtype == crf.dtype == cues.dtype == labels.dtype == np.float32
        assert not ref.has_ties(prob)
        assert set(np.unique(cues)) <= {0.0, 1.0}
        if shape[0] >= 2:
            assert cues[1].sum() == 0 and labels[0, 1:].all() and not labels[-1, 1:].any()
        assert np.abs(np.exp(crf.astype(np.float64)).sum(-1) - 1).max() < 1e-5


def test_seg_loss_is_exported(built):
    """Fails without the feature: the header declares wsc_seg_loss, the library exports it, _lib binds it."""
    declared = _lib.check_exports()
    assert "wsc_seg_loss" in declared
    assert hasattr(_lib.load(), "wsc_seg_loss") and "wsc_seg_loss" in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["wsc_seg_loss"][1]) == 18
    assert _lib.SEG_LOSS_SLOTS == ref.KEYS
