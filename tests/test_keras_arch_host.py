"""CPU: the host side of the Keras-side pooling geometry -- net.common.pooled_size against sizes worked out by hand, the oracle's
own pool, keras_store.read_architecture on architecture files written here, and cues.get_grad_cam_weights with a spec against
torch.autograd on the restated nets (tests/keras_arch_ref.py)."""
import copy
import json

import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import keras_arch_ref as kref
from wsscam import keras_store
from wsscam.cues import utilities as cues
from wsscam.net import common

ALPHA_TOL = 2e-5  # relative to max|alpha|: the bar tests/test_cues_host.py holds the closed forms to


# ---- (a) the size rule --------------------------------------------------------------------------------------------------------
SIZE_TABLE = [
    ((3, 2, "same"), 321, [161, 81, 41]),
    ((2, 2, "same"), 321, [161, 81, 41]), ((2, 2, "same"), 224, [112, 56, 28]), ((2, 2, "same"), 65, [33, 17, 9]),
    ((2, 2, "valid"), 321, [160, 80, 40]), ((2, 2, "valid"), 224, [112, 56, 28]), ((2, 2, "valid"), 65, [32, 16, 8]),
    ((3, 2, "valid"), 321, [160, 79, 39]), ((3, 2, "valid"), 224, [111, 55, 27]),
]


@pytest.mark.parametrize("row,n,sizes", SIZE_TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pooled_size_table(row, n, sizes):
    for i, want in enumerate(sizes):
        assert common.pooled_size(n, [row] * (i + 1)) == want
    assert common.pooled_size(n, []) == n


def test_pool_axis_padding():
    want = {((2, 2, "same"), 8): (4, 0, 0), ((2, 2, "same"), 9): (5, 0, 1), ((3, 2, "same"), 8): (4, 0, 1), ((3, 2, "same"), 9): (5, 1, 1),
            ((3, 1, "same"), 9): (9, 1, 1), ((2, 1, "same"), 9): (9, 0, 1), ((2, 2, "valid"), 9): (4, 0, 0), ((3, 2, "valid"), 8): (3, 0, 0)}
    for (row, n), triple in want.items():
        assert common.pool_axis(n, *row) == triple, (row, n)
        assert kref.tf_pool_axis(n, row[0], row[1], row[2] == "same") == triple, (row, n)  # the oracle's own statement
    for k in (2, 3):
        with pytest.raises(ValueError):
            common.pool_axis(k - 1, k, 1, "valid")
        with pytest.raises(ValueError):
            common.pooled_size(k - 1, [(k, 2, "valid")])
    with pytest.raises(ValueError):
        common.pool_axis(9, 2, 2, "full")


def test_normalize_pooling():
    assert common.normalize_pooling(None) is None
    assert common.normalize_pooling([[3, 2, "same"], (2, 2, "valid"), (2.0, 1, "same")]) == [(3, 2, "same"), (2, 2, "valid"), (2, 1, "same")]
    for bad in ([(3, 2, "same")] * 2, [(4, 2, "same")] * 3, [(3, 3, "same")] * 3, [(2.5, 2, "same")] * 3, [(3, 2, "SAME")] * 3,
                [(3, 2)] * 3):
        with pytest.raises(ValueError):
            common.normalize_pooling(bad)


# ---- (b) the oracle's pool ----------------------------------------------------------------------------------------------------
def test_oracle_pool_ignores_padding():
    """An all-negative map: a zero-padded pool would return 0 wherever a window touches the border."""
    t = torch.tensor([[[[-1.0, -2.0, -3.0], [-4.0, -5.0, -6.0], [-7.0, -8.0, -9.0]]]])
    assert kref.tf_max_pool_t(t, 3, 2, True).tolist() == [[[[-1.0, -2.0], [-4.0, -5.0]]]]   # pad 1 / 1: windows centred on the corners
    assert kref.tf_max_pool_t(t, 2, 2, True).tolist() == [[[[-1.0, -3.0], [-7.0, -9.0]]]]   # pad 0 / 1
    assert kref.tf_max_pool_t(t, 3, 1, True).tolist() == [[[[-1.0, -1.0, -2.0], [-1.0, -1.0, -2.0], [-4.0, -4.0, -5.0]]]]
    assert kref.tf_max_pool_t(t, 2, 2, False).tolist() == [[[[-1.0]]]]                        # row and column 2 are dropped
    assert kref.tf_max_pool_t(t, 2, 1, False).tolist() == [[[[-1.0, -2.0], [-4.0, -5.0]]]]
    assert kref.tf_max_pool_t(t, 3, 2, False).tolist() == [[[[-1.0]]]]
    with pytest.raises(ValueError):
        kref.tf_max_pool_t(t[:, :, :2], 3, 1, False)


# ---- (c) the architecture reader ----------------------------------------------------------------------------------------------
def _write(tmp_path, doc, name="sess.json"):
    p = tmp_path / name
    p.write_text(json.dumps(doc))
    return str(p)


@pytest.mark.parametrize("container", ["list", "dict"])
@pytest.mark.parametrize("batchnorm", [True, False])
@pytest.mark.parametrize("model_type,root", [("VGG16", "vgg16"), ("M7", "m7")])
def test_read_architecture(tmp_path, model_type, root, batchnorm, container):
    pools = [(3, 2, "same"), (2, 2, "valid"), (2, 1, "same")]
    layers = [{"class_name": "InputLayer", "config": {"batch_input_shape": [None, 224, 224, 3]}}] if container == "dict" else []
    layers += kref.keras_layers(root, pools, batchnorm, use_bias=root == "m7")
    got = keras_store.read_architecture(_write(tmp_path, kref.keras_document(layers, container)), model_type)
    assert got == (pools, batchnorm)
    # `strides: null` is Keras' "same as pool_size"
    for l in layers:
        if l["class_name"] == "MaxPooling2D" and l["config"]["pool_size"] == [2, 2] and l["config"]["padding"] == "valid":
            l["config"]["strides"] = None
    assert keras_store.read_architecture(_write(tmp_path, kref.keras_document(layers, container)), model_type) == (pools, batchnorm)


def _first(layers, name, nth=0):
    return [l for l in layers if l["class_name"] == name][nth]["config"]


def _mutations():
    def filters(ls):
        _first(ls, "Conv2D", 2)["filters"] = 96

    def kernel5(ls):
        _first(ls, "Conv2D", 1)["kernel_size"] = [5, 5]

    def fused_relu(ls):
        _first(ls, "Conv2D", 0)["activation"] = "relu"

    def nonsquare_pool(ls):
        _first(ls, "MaxPooling2D", 1)["pool_size"] = [2, 3]

    def no_dense(ls):
        del ls[-1]

    def avg_pool(ls):
        [l for l in ls if l["class_name"] == "MaxPooling2D"][0]["class_name"] = "AveragePooling2D"

    def bn_eps(ls):
        _first(ls, "BatchNormalization", 3)["epsilon"] = 1e-5

    def bn_missing_once(ls):
        del ls[[i for i, l in enumerate(ls) if l["class_name"] == "BatchNormalization"][2]]

    def wrong_global(ls):
        for l in ls:
            if l["class_name"].startswith("Global"):
                l["class_name"] = "Flatten"

    def dense_bias(ls):
        ls[-1]["config"]["use_bias"] = not ls[-1]["config"]["use_bias"]

    def pool_window4(ls):
        _first(ls, "MaxPooling2D", 0)["pool_size"] = [4, 4]

    return {f.__name__: f for f in (filters, kernel5, fused_relu, nonsquare_pool, no_dense, avg_pool, bn_eps, bn_missing_once,
                                    wrong_global, dense_bias, pool_window4)}


@pytest.mark.parametrize("what", sorted(_mutations()))
@pytest.mark.parametrize("model_type,root", [("VGG16", "vgg16"), ("M7", "m7")])
def test_read_architecture_rejects(tmp_path, model_type, root, what):
    pools = [(3, 2, "same")] * 3
    layers = copy.deepcopy(kref.keras_layers(root, pools, True, use_bias=root == "m7"))
    good = _write(tmp_path, kref.keras_document(layers), "good.json")
    assert keras_store.read_architecture(good, model_type) == (pools, True)
    _mutations()[what](layers)
    with pytest.raises(ValueError) as ei:
        keras_store.read_architecture(_write(tmp_path, kref.keras_document(layers)), model_type)
    assert "layer" in str(ei.value) or "ends after" in str(ei.value), str(ei.value)


def test_read_architecture_rejects_functional_model_and_other_type(tmp_path):
    layers = kref.keras_layers("m7", [(2, 2, "valid")] * 3, True, True)
    with pytest.raises(ValueError) as ei:
        keras_store.read_architecture(_write(tmp_path, kref.keras_document(layers, "dict", class_name="Model")), "M7")
    assert "Sequential" in str(ei.value)
    # an M7 file is no VGG16 session (and the other way round): the table decides, never a fallback
    with pytest.raises(ValueError):
        keras_store.read_architecture(_write(tmp_path, kref.keras_document(layers)), "VGG16")
    with pytest.raises(ValueError):
        keras_store.read_architecture(_write(tmp_path, kref.keras_document(kref.keras_layers("vgg16", [(2, 2, "valid")] * 3, True, False))), "M7")


# ---- (d) Grad-CAM alpha with a spec ---------------------------------------------------------------------------------------------
ALPHA_CASES = [("m7", 36, (3, 2, "same")), ("m7", 36, (2, 2, "valid")), ("vgg16", 33, (3, 2, "same")), ("m7", 34, (3, 2, "same"))]


def _alpha_case(root, S, row):
    C = 7
    cfg = cnn_ref.VGG16_CFG if root == "vgg16" else cnn_ref.M7_CFG
    sd = cnn_ref.make_plain_state_dict(root, cfg, C, True, seed=11)
    bn = cnn_ref.last_bn_key(sd, root, cfg)
    sd[bn + ".weight"][::3] *= -1.0  # (negative BatchNorm scales, as tests/test_cues_host.py has them)

    class Model:  # what cues.get_grad_cam_weights reads off a CAM wrapper
        _sd = {k: v.numpy() for k, v in sd.items()}

    Model.root = root
    Model.pooling = common.normalize_pooling([row] * 3)
    ref = kref.grad_cam_weights(sd, root, cfg, S, C, [row] * 3)
    return Model, ref


@pytest.mark.parametrize("root,S,row", ALPHA_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grad_cam_alpha_with_pooling_vs_autograd(root, S, row):
    Model, ref = _alpha_case(root, S, row)
    alpha = cues.get_grad_cam_weights(Model, cues.find_final_layer(Model), np.zeros((1, S, S, 3), np.float32))
    err = np.abs(alpha - ref).max() / np.abs(ref).max()
    print("%s S=%d %s: alpha within %.3g of the autograd alpha (relative to its max)" % (root, S, row, err))
    assert alpha.shape == ref.shape
    assert err <= ALPHA_TOL


def test_grad_cam_alpha_halved_size_is_another_alpha():
    """M7 at 34 under 3 x 3 / 2 SAME pools: A is 9 x 9, the hard-coded halving says 8 x 8; alpha of the global-max head goes
    with 1 / sqrt(h w) through its RMS.  Asserted on the oracle: its alpha is more than 100 x the bar away from the closed
    form at the halved size -- which is what the model without a spec computes."""
    Model, ref = _alpha_case("m7", 34, (3, 2, "same"))
    assert common.pooled_size(34, Model.pooling[:2]) == 9 and 34 // 4 == 8
    Model.pooling = None
    halved = cues.get_grad_cam_weights(Model, cues.find_final_layer(Model), np.zeros((1, 34, 34, 3), np.float32))
    diff = np.abs(halved - ref).max() / np.abs(ref).max()
    print("alpha at the halved size is %.3g away from the oracle's" % diff)
    assert diff > 100 * ALPHA_TOL


# ---- the wrappers keep the spec and hand it to the library's state dict (no device: nothing is packed here) -------------------
def test_wrapper_pooling_plumbing():
    from wsscam.net import m7_cam, vgg16_cam

    sd = {k: v.numpy() for k, v in cnn_ref.make_plain_state_dict("m7", cnn_ref.M7_CFG, 5, True, seed=1).items()}
    m = m7_cam.CAM(None, "voc12", "M7", 5, None, pooling=[(3, 2, "same")] * 3)
    m.load_state_dict(sd)
    ext = m._extra_tensors(m._sd)
    assert np.array_equal(ext["pool_spec"], np.array([[3, 2, 1]] * 3, np.float32)) and ext["pool_spec"].dtype == np.float32
    h = common.pooled_size(m.keras_input_size, m.pooling[:2])
    assert h == 56
    m.keras_input_size = 34  # (a size where the spec's map is not the halved one: 9, not 8)
    want = common.grad_cam_alpha(sd["m7.classifier.0.weight"], 9, 9, "max", bn_scale=common.last_bn_affine(sd, "m7")[0])
    assert np.array_equal(m._extra_tensors(m._sd)["gradcam_weights"], want.astype(np.float32))
    m.set_pooling(None)
    ext = m._extra_tensors(m._sd)
    assert "pool_spec" not in ext
    want = common.grad_cam_alpha(sd["m7.classifier.0.weight"], 8, 8, "max", bn_scale=common.last_bn_affine(sd, "m7")[0])
    assert np.array_equal(ext["gradcam_weights"], want.astype(np.float32))
    v = vgg16_cam.CAM(None, "voc12", "VGG16", 5, None)
    assert v.pooling is None and v._with_pool_spec({"a": 1}) == {"a": 1}
    v.set_pooling([(2, 2, "valid"), (3, 2, "same"), (3, 1, "valid")])
    assert np.array_equal(v._with_pool_spec({})["pool_spec"], np.array([[2, 2, 0], [3, 2, 1], [3, 1, 0]], np.float32))
    with pytest.raises(ValueError):
        v.set_pooling([(2, 2, "valid")])
    with pytest.raises(TypeError):
        vgg16_cam.CAM(None, "voc12", "VGG16", 5, None, None, [(2, 2, "valid")] * 3)  # keyword-only
