"""CPU: the oracle of the 01_train dropout sites (tests/cls_dropout_ref.py) against torch itself, and keras_store.read_dropout.

  chain_grads_drop on a float64 tape IS whole-graph autograd of the forward pass with explicit mask multiplication, for both stacks,
  with and without BatchNorm (the BatchNorm sites take their masks from keep_mask, the post-ReLU sites from the tape);
  drop_prob = 0 reproduces tests/cls_grad_ref.py exactly; the sites are numbered by the `D` entries of the tables;
  M7's site in front of the global max: a dropped +0.0 wins the maximum of an all-negative channel and passes no gradient on;
  R32_CHAIN_CLS_DROP, the float32 evaluation's own error on one float32 tape, is re-measured and held to 1.5 x its recorded value."""
import json

import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import cls_dropout_ref as dref
from tests import cls_grad_ref as gref
from tests.test_cls_grad_oracle import THIN
from wsscam import keras_store
from wsscam.net import common

THIN_CASES = [("vgg16", True, None, (33, 33)), ("vgg16", False, gref.KERAS_POOLS, (40, 24)), ("m7", True, gref.KERAS_POOLS, (17, 21)),
              ("m7", False, None, (12, 12))]


@pytest.fixture
def thin(monkeypatch):
    monkeypatch.setattr(gref, "CFG", THIN)


@pytest.mark.parametrize("drop_prob", [0.5, 0.3])
@pytest.mark.parametrize("case", THIN_CASES, ids=gref.case_id)
def test_chain_on_a_float64_tape_is_autograd(thin, case, drop_prob):
    root, bn, pools, hw = case
    drop = (drop_prob, 11, 2)
    sd = cnn_ref.make_plain_state_dict(root, THIN[root], 5, bn, seed=3)
    x = gref.net_input(hw)
    tape, feat = dref.forward_tape_drop(root, sd, x, pools, drop)
    plain_tape, plain_feat = gref.forward_tape(root, sd, x, pools)
    assert sorted(tape) == sorted(plain_tape)  # no mask entry, the same names
    if root == "m7":  # the pooled map, with zeros where dropped
        assert feat.shape == gref._nhwc(dref.head_pool_t(gref._nchw(plain_feat, torch.float64), pools)).shape != plain_feat.shape
    assert (feat == 0).mean() > 0.5 * drop_prob
    dfeat = np.random.default_rng(5).standard_normal(feat.shape)
    want = dref.autograd_grads_drop(root, sd, x, dfeat, pools, drop)
    got = dref.chain_grads_drop(root, sd, tape, dfeat, pools, drop)
    assert list(got) and sorted(got) == sorted(want) == sorted(gref.param_names(root, sd))
    worst = gref.worst_ratio(got, want)
    print("chain vs autograd with dropout %s p=%.1f: worst max|d| / max|g| %.3e at %s" % ((gref.case_id(case), drop_prob) + worst))
    assert worst[0] <= 1e-12  # the tolerance of tests/test_cls_grad_oracle.py for the same statement
    for n, w in want.items():
        assert np.abs(w).max() > 0, n
    # it is another gradient than the one without dropout
    assert gref.worst_ratio(gref.autograd_grads(root, sd, x, np.ones_like(plain_feat), pools),
                            dref.autograd_grads_drop(root, sd, x, np.ones_like(feat), pools, drop))[0] > 1e-3


@pytest.mark.parametrize("case", THIN_CASES, ids=gref.case_id)
def test_drop_prob_zero_is_the_pass_without_dropout(thin, case):
    root, bn, pools, hw = case
    sd = cnn_ref.make_plain_state_dict(root, THIN[root], 5, bn, seed=3)
    x = gref.net_input(hw)
    tape, feat = dref.forward_tape_drop(root, sd, x, pools, (0.0, 11, 2))
    want_tape, want_feat = gref.forward_tape(root, sd, x, pools)
    assert np.array_equal(feat, want_feat) and all(np.array_equal(tape[k], want_tape[k]) for k in want_tape)
    dfeat = np.random.default_rng(5).standard_normal(feat.shape)
    got, want = dref.chain_grads_drop(root, sd, tape, dfeat, pools, (0.0, 11, 2)), gref.chain_grads(root, sd, want_tape, dfeat, pools)
    assert all(np.array_equal(got[n], want[n]) for n in want)
    auto = dref.autograd_grads_drop(root, sd, x, dfeat, pools, (0.0, 11, 2))
    assert all(np.array_equal(auto[n], w) for n, w in gref.autograd_grads(root, sd, x, dfeat, pools).items())
    # a mask of drop_prob = 0 keeps everything at scale 1
    assert dref.keep_mask((3, 5), 0.0, 11, 2, 0).all() and dref.scale_of(0.0) == 1.0


def test_site_numbering():
    """by the order of the `D` entries of the tables: VGG16 0 and 1 behind the two entries of layer5 (state-dict indices differ with
    BatchNorm), M7's one in the classifier branch; the package's table agrees"""
    for bn, names in ((True, ("vgg16.layer5.0", "vgg16.layer5.4")), (False, ("vgg16.layer5.0", "vgg16.layer5.3"))):
        sd = gref.state_dict("vgg16", bn)
        assert dref.drop_sites("vgg16", sd) == {names[0]: 0, names[1]: 1}
        last_two = [n for k, n, _ in gref.stack_ops("vgg16", sd) if k == "conv"][-2:]
        assert last_two == list(names)
    for bn in (True, False):
        assert dref.drop_sites("m7", gref.state_dict("m7", bn)) == {}  # none inside the stack
    assert dref.M7_SITE == 0
    assert common.DROP_SITES == {"vgg16": 2, "m7": 1}
    assert sum(v == "D" for _, layer in common.PLAIN_CFG["vgg16"] for v in layer) == 2
    # two sites of one pass draw different masks, and so do two steps
    m0, m1 = dref.keep_mask((4, 8), 0.5, 7, 3, 0), dref.keep_mask((4, 8), 0.5, 7, 3, 1)
    assert (m0 != m1).any() and (m0 != dref.keep_mask((4, 8), 0.5, 7, 4, 0)).any()


def test_m7_dropped_zero_wins_the_global_max():
    """a hand-built layer3_p1 map: channel 0 all negative, channel 1 positive.  Behind pool -> mask the dropped elements of channel 0
    are +0.0, the maximum of the channel; the global max sends its gradient there, the site multiplies it by 0: nothing reaches the
    channel's input.  Channel 1's maximum is a kept value and its gradient arrives."""
    drop = (0.5, 7, 3)
    rng = np.random.default_rng(4)
    x = np.stack([-1.0 - rng.random((1, 6, 8)), 1.0 + rng.random((1, 6, 8))], axis=-1)  # NHWC (1, 6, 8, 2)
    keep = dref.keep_mask((1, 3, 4, 2), *drop, dref.M7_SITE)
    assert not keep[..., 0].all() and keep[..., 1].any()  # channel 0 has a dropped element
    xt = gref._nchw(x, torch.float64).requires_grad_(True)
    d = dref.m7_head_t(xt, None, drop)
    top = d.amax(dim=(2, 3))
    assert top[0, 0] == 0.0 and top[0, 1] > 2.0  # the dropped zero is channel 0's maximum; channel 1's is a kept value times 2
    top.sum().backward()
    g = gref._nhwc(xt.grad)
    assert not g[..., 0].any() and np.count_nonzero(g[..., 1]) == 1 and g[..., 1].max() == 2.0
    # the chain form: the loss head's gradient on the dropped map (1 at each channel's first maximum), then the site and the pool
    dn = gref._nhwc(d)
    dfeat = np.zeros_like(dn)
    for c in range(2):
        dfeat.reshape(-1, 2)[np.argmax(dn.reshape(-1, 2)[:, c]), c] = 1.0
    assert not keep.reshape(-1, 2)[np.argmax(dn.reshape(-1, 2)[:, 0]), 0]  # it sits on a dropped element
    gc = gref._nhwc(dref.m7_head_grad_t(gref._nchw(x, torch.float64), gref._nchw(dfeat, torch.float64), None, drop))
    assert np.array_equal(gc, g)


def test_float32_chain_error():
    """R32_CHAIN_CLS_DROP: chain_grads_drop in float32 against float64 on one float32 tape, over the GPU cases at drop_prob = 0.5"""
    worst = (0.0, "", "")
    for case in dref.DROP_CASES:
        root, bn, pools, hw = case
        sd = gref.state_dict(root, bn)
        tape32, feat = dref.forward_tape_drop(root, sd, gref.net_input(hw), pools, dref.DROP, dtype=torch.float32)
        dfeat = gref.case_dfeat(case, feat.shape)
        g64 = dref.chain_grads_drop(root, sd, tape32, dfeat, pools, dref.DROP, dtype=torch.float64)
        g32 = dref.chain_grads_drop(root, sd, tape32, dfeat, pools, dref.DROP, dtype=torch.float32)
        r = gref.worst_ratio(g32, g64)
        print("float32 chain with dropout %s: worst max|g32 - g64| / max|g64| %.3e at %s" % ((gref.case_id(case),) + r))
        worst = max(worst, r + (gref.case_id(case),))
    print("R32_CHAIN_CLS_DROP measured %.3e (%s of %s), recorded %.3e" % (worst + (dref.R32_CHAIN_CLS_DROP,)))
    assert 0 < worst[0] <= 1.5 * dref.R32_CHAIN_CLS_DROP


# ---- keras_store.read_dropout on hand-written architecture files --------------------------------------------------------------------
def _doc(path, layers):
    path.write_text(json.dumps({"class_name": "Sequential", "config": {"layers": [{"class_name": n, "config": c} for n, c in layers]}}))
    return str(path)


CONV = ("Conv2D", {"filters": 8})


def test_read_dropout(tmp_path):
    two = [CONV, ("Dropout", {"rate": 0.5}), CONV, ("Dropout", {"rate": 0.5}), ("Dense", {})]
    assert keras_store.read_dropout(_doc(tmp_path / "a.json", two), "VGG16") == 0.5
    assert keras_store.read_dropout(_doc(tmp_path / "b.json", [CONV, ("MaxPooling2D", {}), ("Dropout", {"rate": 0.25}), ("Dense", {})]), "M7") == 0.25
    assert keras_store.read_dropout(_doc(tmp_path / "c.json", [CONV, CONV, ("Dense", {})]), "VGG16") is None  # rates absent
    assert keras_store.read_dropout(_doc(tmp_path / "d.json", [CONV, ("Dense", {})]), "M7") is None
    # the "config" may be the bare layer list
    (tmp_path / "e.json").write_text(json.dumps({"class_name": "Sequential", "config": [{"class_name": "Dropout", "config": {"rate": 0.5}}]}))
    assert keras_store.read_dropout(str(tmp_path / "e.json"), "M7") == 0.5
    # a wrong count names a layer: the one Dropout of a VGG16 (index 1), the second of an M7 (index 3)
    with pytest.raises(ValueError, match="layer 1:"):
        keras_store.read_dropout(_doc(tmp_path / "f.json", two[:2] + [("Dense", {})]), "VGG16")
    with pytest.raises(ValueError, match="layer 3:"):
        keras_store.read_dropout(_doc(tmp_path / "g.json", two), "M7")
    # disagreeing rates name the layer that differs from the first
    with pytest.raises(ValueError, match="layer 3:"):
        keras_store.read_dropout(_doc(tmp_path / "h.json", two[:3] + [("Dropout", {"rate": 0.3}), ("Dense", {})]), "VGG16")
    with pytest.raises(ValueError, match="layer 2:"):  # a rate that is no probability
        keras_store.read_dropout(_doc(tmp_path / "i.json", [CONV, CONV, ("Dropout", {"rate": 1.0})]), "M7")
