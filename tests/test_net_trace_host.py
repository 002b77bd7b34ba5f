"""CPU: the per-op float64 reference of tests/net_trace_ref.py against the whole-network oracles it must add up to.  Chaining the
closures from the network input reproduces oracle/cnn_ref.py (ResNet50 features and CAM; VGG16 with and without BatchNorm; M7)
and the trunk of tests/deeplab_ref.py, each run in double, to 1e-12 max|ref|; the stage-entry closure equals cnn_ref._bottleneck
on odd sizes at stride 2; the label list names every conv weight of the state dict once; and a wrong closure (the mutants the
device tests are meant to catch) lies outside the bound the device is held to."""
import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import deeplab_ref, keras_arch_ref
from tests import net_trace_ref as nt

REL = 1e-12


def _double(sd):
    return {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= REL * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def resnet_sd():
    return cnn_ref.make_resnet50_cam_state_dict(20, seed=0)


@pytest.mark.parametrize("prec", ["f32", "f16x3", "bf16x3"])
def test_resnet50_chain_is_the_oracle(resnet_sd, prec):
    """every wiring of the stage entry (separate projection + residual, two-source GEMM, materialised concatenation)"""
    x = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (2, 3, 33, 49))).double()
    layers = nt.resnet50_layers(resnet_sd, prec)
    outs = nt.chain(layers, x)
    sdd = _double(resnet_sd)
    with torch.no_grad():
        _close(outs[-2], cnn_ref.resnet50_features(x, sdd))
        _close(nt.cam_from_head(outs[-1])[0], cnn_ref.resnet50_cam_forward(x, sdd))
    n_entry = sum(ly.entry for ly in layers)
    assert n_entry == (0 if prec == "f32" else 4) and sum(ly.kind == "gather" for ly in layers) == (4 if prec == "bf16x3" else 0)
    assert len(layers) == {"f32": 2 + 16 * 3 + 4 + 1, "f16x3": 2 + 16 * 3 + 1, "bf16x3": 2 + 16 * 3 + 4 + 1}[prec]
    for i, ly in enumerate(layers):
        assert all(j < i for j in ly.inputs), (i, ly.label, ly.inputs)


@pytest.mark.parametrize("hw", [(9, 13), (17, 25), (8, 8)])
def test_stage_entry_closure_is_the_bottleneck_tail(resnet_sd, hw):
    """relu(bn3(conv3(y2)) + bn_d(conv_d(x[::2, ::2]))) on odd maps: layer2.0 of the oracle, fed the oracle's own conv2 output"""
    sdd = _double(resnet_sd)
    pre = "resnet50.layer2.0"
    x = torch.from_numpy(np.random.default_rng(hw[0]).normal(0, 1, (2, 256) + hw)).double()
    layers = {ly.label: ly for ly in nt.resnet50_layers(resnet_sd, "f16x3")}
    y1 = layers[pre + ".conv1"].fn(x)[0]
    y2 = layers[pre + ".conv2"].fn(y1)[0]
    assert tuple(y2.shape[2:]) == ((hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1)
    got, A, _ = layers[pre + ".conv3+downsample"].fn(y2, x)
    with torch.no_grad():
        want = cnn_ref._bottleneck(x, sdd, pre, 2)
    _close(got, want)
    assert (A >= got.abs() * (1 - 1e-12)).all()  # A is the magnitude the value is made of
    # the materialised form reads the same tensors from one concatenation
    cat = torch.cat([y2, x[:, :, ::2, ::2]], 1)
    _close({ly.label: ly for ly in nt.resnet50_layers(resnet_sd, "bf16x3")}[pre + ".conv3+downsample"].fn(cat)[0], want)
    # ... and a second source one row off is another function
    off = {ly.label: ly for ly in nt.resnet50_layers(resnet_sd, "f16x3", mutate="tap")}[pre + ".conv3+downsample"].fn(y2, x)[0]
    assert (off - want).abs().max() > 1e-2 * want.abs().max()


@pytest.mark.parametrize("root, batchnorm", [("vgg16", True), ("vgg16", False), ("m7", True)])
def test_plain_chain_is_the_oracle(root, batchnorm):
    cfg = cnn_ref.VGG16_CFG if root == "vgg16" else cnn_ref.M7_CFG
    sd = cnn_ref.make_plain_state_dict(root, cfg, 20, batchnorm, seed=2)
    x = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (2, 3, 33, 37))).double()
    outs = nt.chain(nt.plain_layers(sd, root, cfg), x)
    with torch.no_grad():
        _close(outs[-1], cnn_ref.plain_features(x, _double(sd), root, cfg))


def test_m7_chain_with_a_pool_spec_is_the_pooled_oracle():
    pools = [(3, 2, "same"), (2, 2, "valid")]
    sd = cnn_ref.make_plain_state_dict("m7", cnn_ref.M7_CFG, 20, True, seed=4)
    x = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (2, 3, 33, 37))).double()
    layers = nt.plain_layers(sd, "m7", cnn_ref.M7_CFG, pools=[(3, 2, 1), (2, 2, 0)])
    assert [ly.pool for ly in layers if ly.kind == "pool"] == [(nt.POOL_TF_SAME, 3, 2, 0, 0), (nt.POOL_TF_VALID, 2, 2, 0, 0)]
    with torch.no_grad():
        _close(nt.chain(layers, x)[-1], keras_arch_ref.plain_features_pooled(x, _double(sd), "m7", cnn_ref.M7_CFG, pools))


def test_deeplab_trunk_chain_is_the_oracle():
    wts = deeplab_ref.random_weights("SEC", 5, 64, 128, seed=7)
    x = deeplab_ref.net_input(2, 41, 41, 8)
    layers = nt.deeplab_layers(wts)
    out = nt.chain(layers, torch.from_numpy(x).double().permute(0, 3, 1, 2))[-1]
    # the oracle's own trunk: its forward() up to pool5a
    lw = deeplab_ref.layer_weights("SEC", wts)
    t = deeplab_ref._nchw(x, torch.float64)
    for layer in deeplab_ref.TRUNK:
        t = deeplab_ref.conv_t(t, lw[layer][0], lw[layer][1], dil=2 if layer.startswith("conv5") else 1)
        if layer in ("conv1_2", "conv2_2", "conv3_3"):
            t = deeplab_ref.max_pool_same_t(t, 2)
        elif layer in ("conv4_3", "conv5_3"):
            t = deeplab_ref.max_pool_same_t(t, 1)
    _close(out, deeplab_ref.avg_pool_same_t(t))
    assert [ly.pool[2] for ly in layers if ly.kind == "pool"] == [2, 2, 2, 1, 1, 1] and layers[-1].pool[4] == 1


@pytest.mark.parametrize("prec", ["f32", "f16x3", "bf16x3"])
def test_labels_name_every_conv_weight_once(resnet_sd, prec):
    named = [k for ly in nt.resnet50_layers(resnet_sd, prec) for k in ly.weights]
    assert sorted(named) == nt.conv_weight_keys(resnet_sd) and len(set(named)) == len(named)
    labels = [ly.label for ly in nt.resnet50_layers(resnet_sd, prec)]
    assert len(set(labels)) == len(labels)
    for root, cfg in (("vgg16", cnn_ref.VGG16_CFG), ("m7", cnn_ref.M7_CFG)):
        sd = cnn_ref.make_plain_state_dict(root, cfg, 20, True, seed=1)
        named = [k for ly in nt.plain_layers(sd, root, cfg) for k in ly.weights]
        assert sorted(named) == nt.conv_weight_keys(sd)
    wts = deeplab_ref.random_weights("SEC", 5, 64, 128, seed=7)
    sd = {n + ".w": wts[n]["w"] for n in deeplab_ref.TRUNK}
    assert sorted(k for ly in nt.deeplab_layers(wts) for k in ly.weights) == nt.conv_weight_keys(sd)


# ---- the reference side of the mutants: a subtly wrong op is farther from the right one than the bound the device is held to ------
def _worst_ratio(layers_ok, layers_bad, x, prec, only=None):
    """max over the ops `only` selects of |bad - ok| / asserted bound, each op fed the RIGHT chain's operands"""
    outs = nt.chain(layers_ok, x)
    worst = {}
    for i, (ok, bad) in enumerate(zip(layers_ok, layers_bad)):
        if ok.kind != "conv" or (only and not only(ok)):
            continue
        a, b, c = [x if j == nt.INPUT else (None if j == nt.NONE else outs[j]) for j in ok.inputs]
        ref, A, S = [t.numpy() for t in ok.fn(a, b, c)]
        bound, _, _ = nt.asserted_bound(prec, ok, ref, A, S)
        worst[ok.label] = float((np.abs(bad.fn(a, b, c)[0].numpy() - ref) / bound).max())
    return worst


def test_mutant_second_source_one_row_off_exceeds_the_bound():
    sd = nt.extreme_bn_state_dict()
    x = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (1, 3, 65, 97))).double()
    w = _worst_ratio(nt.resnet50_layers(sd, "f16x3", False), nt.resnet50_layers(sd, "f16x3", False, mutate="tap"), x, "f16x3",
                     only=lambda ly: ly.entry)
    print("tap mutant, |bad - ok| / bound per stage entry:", w)
    # (layer1 and layer4 enter at stride 1, where the mutant reads row ho + 1 too)
    assert len(w) == 4 and min(w.values()) > 100


def test_mutant_second_affine_before_the_relu_exceeds_the_bound():
    sd = nt.odd_s2_state_dict()
    x = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (1, 3, 33, 37))).double()
    for prec in ("f32", "f16x3"):
        w = _worst_ratio(nt.plain_layers(sd, "vgg16", cnn_ref.VGG16_CFG), nt.plain_layers(sd, "vgg16", cnn_ref.VGG16_CFG, mutate="affine_before_relu"),
                         x, prec)
        print("affine-before-ReLU mutant (%s), |bad - ok| / bound per layer:" % prec, w)
        assert len(w) == 15 and min(w.values()) > 100


def test_mutant_sigma_from_s3_alone():
    """sigma_c = |s3_c| instead of max(|s3_c|, |sd_c|): where the shortcut's scale is the larger one its weights, times sd / |s3|,
    dominate the channel's power-of-two packing and the conv3 weights beside them lose their lo bits.  The f16x3 weight pairs of
    the right fold stay inside the bound (the bound covers the packing); those of the wrong fold are measured against it."""
    sd = nt.extreme_bn_state_dict()
    x = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (1, 3, 65, 97))).double()
    ok = nt.resnet50_layers(sd, "f16x3", False)
    entry = lambda ly: ly.entry
    w_ok = _worst_ratio(ok, nt.resnet50_layers(sd, "f16x3", False, mutate="split"), x, "f16x3", only=entry)
    w_bad = _worst_ratio(ok, nt.resnet50_layers(sd, "f16x3", False, mutate="sigma"), x, "f16x3", only=entry)
    print("f16x3 weight pairs of the right fold, distance / bound:", w_ok)
    print("sigma = |s3| mutant, distance / bound:", w_bad)
    assert max(w_ok.values()) <= 1.0
