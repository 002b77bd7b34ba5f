"""GPU: the MaxPooling2D geometry of a Keras-side session (`pool_spec`) -- the TF max pool (csrc/pool.hip, through
wsc_pool_tf_nhwc), the VGG16 / M7 CAM nets built with a spec against the torch-CPU oracle tests/keras_arch_ref.py, the key's
validation in wsc_net_create, and keras_store.load_model reading a session's architecture file.

Bars.  A maximum returns one of its inputs and adds no rounding: the kernel is held to equality on inputs the activation planes
hold exactly, and the nets to the bars the fixed architectures have in tests/test_gpu_net.py (restated below)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import keras_arch_ref as kref
from wsscam import _lib
from wsscam.net import common, m7_cam, vgg16_cam

pytestmark = pytest.mark.gpu

# tests/test_gpu_net.py: |cam - ref| <= TOL_RAW * max(ref); test_vgg16_cam's score bars; test_m7_cam's tolerances
TOL_RAW = {_lib.PREC_BF16: 3e-2, _lib.PREC_F16: 5e-3, _lib.PREC_BF16X3: 2e-4, _lib.PREC_F16X3: 2e-5}
TOL_SCORE = {_lib.PREC_BF16: 5e-3, _lib.PREC_F16: 1e-3, _lib.PREC_BF16X3: 1e-4, _lib.PREC_F16X3: 2e-5}
PRECISIONS = [_lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_BF16X3, _lib.PREC_F16X3]
TOL_M7 = {_lib.PREC_F16X3: 1e-4, _lib.PREC_BF16X3: 2e-4}

SAME3, VALID2 = [(3, 2, "same")] * 3, [(2, 2, "valid")] * 3


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
POOL_SIZES = [(9, 9), (8, 6), (1, 5), (2, 3), (33, 17)]
GEOMETRIES = [(k, s, same) for k in (2, 3) for s in (1, 2) if s <= k for same in (0, 1)]


def _pool(ctx, x, k, stride, same, prec):
    N, H, W, C = x.shape
    x_dev = ctx.to_device(x)
    try:
        y_dev, shp = _lib.pool_tf_nhwc(ctx, x_dev, N, H, W, C, k, stride, same, prec)
        y = ctx.to_host(y_dev, shp, np.float32)
        y_dev.free()
        return y
    finally:
        x_dev.free()


def _split_representable(x):
    """the nearest value an (f16 hi, f16 lo) pair holds (tests/test_gpu_deeplab.py)"""
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32) + lo.astype(np.float32)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()


def _bf16_split_representable(x):
    hi = _bf16(x)
    return hi + _bf16(x - hi)


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("hw", POOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_pool_tf_kernel(ctx, hw, C):
    """Signed inputs (a zero-padded pool would pass unnoticed after a ReLU), every geometry, every activation layout."""
    rng = np.random.default_rng(hw[0] * 100 + hw[1] + C)
    shape = (2,) + hw + (C,)
    x = (rng.normal(0, 3, shape) - 1.0).astype(np.float32)
    x[..., 0] = -np.abs(x[..., 0]) - 0.5  # every window of channel 0 is all-negative
    inputs = {_lib.PREC_F32: x, _lib.PREC_F16X3: _split_representable(x), _lib.PREC_F16: x.astype(np.float16).astype(np.float32),
              _lib.PREC_BF16: _bf16(x), _lib.PREC_BF16X3: _bf16_split_representable(x)}
    assert np.array_equal(_split_representable(inputs[_lib.PREC_F16X3]), inputs[_lib.PREC_F16X3])
    assert np.array_equal(_bf16_split_representable(inputs[_lib.PREC_BF16X3]), inputs[_lib.PREC_BF16X3])
    n_ok = 0
    for k, stride, same in GEOMETRIES:
        fits = same or (hw[0] >= k and hw[1] >= k)
        for prec, xin in inputs.items():
            if not fits:
                with pytest.raises(_lib.WscError) as ei:
                    _pool(ctx, xin, k, stride, same, prec)
                assert ei.value.status == _lib.WSC_ERR_INVALID, (k, stride, same, prec)
                continue
            r = kref.tf_max_pool(xin, k, stride, same)
            want_hw = tuple(common.pooled_size(n, [(k, stride, "same" if same else "valid")]) for n in hw)
            y = _pool(ctx, xin, k, stride, same, prec)
            assert y.shape == r.shape == (2,) + want_hw + (C,), (k, stride, same, prec, y.shape, r.shape)
            assert np.array_equal(y.astype(np.float64), r), (k, stride, same, prec, np.abs(y - r).max())
            assert (r[..., 0] < 0).all()  # (all-negative windows exist: zero padding would show)
            n_ok += 1
    assert n_ok >= 4 * len(inputs)  # (the four SAME geometries fit every size)
    ctx.sync()


def test_pool_tf_entry_rejects(ctx):
    x = np.zeros((1, 4, 4, 8), np.float32)
    for k, stride, same in ((4, 2, 1), (1, 1, 1), (3, 3, 1), (2, 0, 0), (3, 2, 2)):
        with pytest.raises(_lib.WscError) as ei:
            _pool(ctx, x, k, stride, same, _lib.PREC_F16X3)
        assert ei.value.status == _lib.WSC_ERR_INVALID, (k, stride, same)
    with pytest.raises(_lib.WscError) as ei:
        _pool(ctx, np.zeros((1, 4, 4, 12), np.float32), 2, 2, 0, _lib.PREC_F16X3)  # C not a multiple of 8
    assert ei.value.status == _lib.WSC_ERR_INVALID


# ---- 2. VGG16 -------------------------------------------------------------------------------------------------------------------
def _model(cls, sd, C, precision, pooling=None):
    m = cls(None, "voc12", "", C, None, precision=precision, pooling=pooling)
    m.load_state_dict(sd)
    return m.eval().cuda(0)


@functools.lru_cache(maxsize=None)
def _vgg_case(batchnorm):
    """(state dict, input pair, {pooling: (cam, score)} of the oracle) -- computed once, shared by the precisions"""
    C = 20
    sd = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, batchnorm, seed=1)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(np.random.default_rng(4), 80, 90), (65, 65))
    refs = {}
    with torch.no_grad():
        for name, pools in (("same3", SAME3), ("valid2", VALID2)):
            cam, score = kref.vgg16_cam_forward(torch.from_numpy(x), sd, C, pools)
            refs[name] = (cam.numpy(), score.numpy())
        # the oracle with 2 x 2 / 2 VALID rows IS the fixed architecture's oracle
        cam0, score0 = cnn_ref.vgg16_cam_forward(torch.from_numpy(x), sd, C)
    assert np.array_equal(refs["valid2"][0], cam0.numpy()) and np.array_equal(refs["valid2"][1], score0.numpy())
    return sd, x, refs


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("batchnorm", [True, False])
def test_vgg16_cam_with_pool_spec(precision, batchnorm):
    C = 20
    sd, x, refs = _vgg_case(batchnorm)
    out = {}
    for name, pools in (("same3", SAME3), ("valid2", VALID2), ("none", None)):
        model = _model(vgg16_cam.CAM, sd, C, precision, pools)
        out[name] = model.forward_batch(x[None], want_score=True)
        assert model.cam_size(65) == (9 if name == "same3" else 8)
        assert model.cam_size_hw(65, 33) == ((9, 5) if name == "same3" else (8, 4))
    # 2 x 2 / 2 VALID given explicitly: the fixed architecture's output, bit for bit (another kernel, the same maxima)
    assert out["valid2"][0].shape == (1, C, 8, 8)
    assert np.array_equal(out["valid2"][0], out["none"][0]) and np.array_equal(out["valid2"][1], out["none"][1])
    for name, hw in (("same3", 9), ("valid2", 8)):
        (cam, score), (rcam, rscore) = out[name], refs[name]
        assert cam[0].shape == rcam.shape == (C, hw, hw)
        e_cam, e_score = np.abs(cam[0] - rcam).max() / float(rcam.max()), np.abs(score[0] - rscore).max()
        print("vgg16 %s bn=%d prec=%d: cam %.3g of max (bar %.3g), score %.3g (bar %.3g)" % (name, batchnorm, precision, e_cam,
                                                                                             TOL_RAW[precision], e_score, TOL_SCORE[precision]))
        assert e_cam <= TOL_RAW[precision]
        assert e_score <= TOL_SCORE[precision]
    # the two geometries are different networks: the oracle's own maps differ in size, so nothing above passes by accident
    assert refs["same3"][0].shape != refs["valid2"][0].shape


# ---- 3. M7 ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _m7_case(S, same):
    C = 20
    pools = SAME3 if same else VALID2
    sd = cnn_ref.make_plain_state_dict("m7", cnn_ref.M7_CFG, C, True, seed=2)
    alpha = kref.grad_cam_weights(sd, "m7", cnn_ref.M7_CFG, S, C, pools)  # (F, C)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(np.random.default_rng(5), 70, 60), (S, S))
    with torch.no_grad():
        cam, score = kref.m7_cam_forward(torch.from_numpy(x), sd, torch.from_numpy(alpha), C, pools)
        _, score_nocrop = kref.m7_cam_forward(torch.from_numpy(x), sd, torch.from_numpy(alpha), C, pools, crop=False)
    return sd, alpha, x, pools, cam.numpy(), score.numpy(), score_nocrop.numpy()


@pytest.mark.parametrize("precision", [_lib.PREC_F16X3, _lib.PREC_BF16X3])
@pytest.mark.parametrize("S,same,hw", [(64, True, 16), (36, False, 9)], ids=["64-same3", "36-valid2-cropped"])
def test_m7_cam_with_pool_spec(precision, S, same, hw):
    """36 under 2 x 2 / 2 VALID: 18 -> 9, and the classifier branch's pool 9 -> 4 leaves row and column 8 out -- the reference's
    score is the maximum of the pooled map, not of the map (30 % of the 256 channels have their maximum in what is dropped: 77, sample 0)."""
    C, tol = 20, TOL_M7[precision]
    sd, alpha, x, pools, rcam, rscore, rscore_nocrop = _m7_case(S, same)
    if same:
        assert np.array_equal(rscore, rscore_nocrop)  # a SAME pool covers every position
    else:
        moved = np.abs(rscore - rscore_nocrop).max()
        print("oracle: cropped and uncropped scores differ by %.3g (tolerance %.3g)" % (moved, tol))
        assert moved >= 100 * tol
    sd_dev = dict(sd)
    sd_dev["gradcam_weights"] = torch.from_numpy(alpha.astype(np.float32))
    model = _model(m7_cam.CAM, sd_dev, C, precision, pools)
    cam, score = model.forward_batch(x[None], want_score=True)
    assert cam[0].shape == rcam.shape == (C, hw, hw) and model.cam_size(S) == hw
    e_cam, e_score = np.abs(cam[0] - rcam).max() / max(float(rcam.max()), 1e-3), np.abs(score[0] - rscore).max()
    print("m7 S=%d %s prec=%d: cam %.3g, score %.3g (tolerance %.3g)" % (S, pools[0], precision, e_cam, e_score, tol))
    assert e_cam <= tol
    assert e_score <= tol
    # the plain-batch entry (wsc_net_forward_gradcam) runs the same classifier branch
    from wsscam.cues import utilities as cues

    imgs = np.ascontiguousarray(np.transpose(x[:1], (0, 2, 3, 1)))
    _, scores = cues.conv_and_cams(model, alpha.astype(np.float32), imgs, relu=True, want_scores=True)
    assert np.abs(scores[0] - rscore).max() <= tol


# ---- 4. the key's validation ----------------------------------------------------------------------------------------------------
def test_pool_spec_errors(ctx):
    C = 20
    sd = {k: v.numpy() for k, v in cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, True, seed=1).items()}

    def status(arch, spec, what):
        bad = dict(sd)
        bad["pool_spec"] = np.asarray(spec, np.float32)
        with pytest.raises(_lib.WscError) as ei:
            _lib.Net(ctx, arch, bad, C)
        print(what, "->", ei.value)
        return ei.value.status, str(ei.value)

    assert status(_lib.ARCH_VGG16_CAM, [[2, 2, 0]] * 2, "two rows")[0] == _lib.WSC_ERR_SHAPE
    assert status(_lib.ARCH_VGG16_CAM, [2, 2, 0] * 3, "a flat tensor")[0] == _lib.WSC_ERR_SHAPE
    st, msg = status(_lib.ARCH_VGG16_CAM, [[2, 2, 0], [4, 2, 1], [2, 2, 0]], "window 4")
    assert st == _lib.WSC_ERR_INVALID and "row 1" in msg
    st, msg = status(_lib.ARCH_VGG16_CAM, [[3, 2, 0], [3, 2, 1], [3, 3, 0]], "stride 3")
    assert st == _lib.WSC_ERR_INVALID and "row 2" in msg
    st, msg = status(_lib.ARCH_VGG16_CAM, [[2.5, 2, 0], [2, 2, 1], [2, 2, 0]], "a non-integral window")
    assert st == _lib.WSC_ERR_INVALID and "row 0" in msg
    assert status(_lib.ARCH_VGG16_CAM, [[2, 2, 0], [2, 2, 2], [2, 2, 0]], "same = 2")[0] == _lib.WSC_ERR_INVALID
    assert status(_lib.ARCH_VGG16_IRN, [[2, 2, 0]] * 3, "an IRN flavour")[0] == _lib.WSC_ERR_INVALID
    # a valid spec on the same tensors builds
    ok = dict(sd)
    ok["pool_spec"] = np.asarray([[3, 2, 1]] * 3, np.float32)
    net = _lib.Net(ctx, _lib.ARCH_VGG16_CAM, ok, C)
    assert net.cam_size(321) == 41 and net.cam_size(65) == 9
    with pytest.raises(_lib.WscError) as ei:  # 3 x 3 VALID pools do not fit a 9 x 9 input's 3 -> 1 map
        ok["pool_spec"] = np.asarray([[3, 2, 0]] * 3, np.float32)
        _lib.Net(ctx, _lib.ARCH_VGG16_CAM, ok, C).cam_size(9)
    assert ei.value.status == _lib.WSC_ERR_INVALID
    net.close()


# ---- 5. the driver --------------------------------------------------------------------------------------------------------------
def _keras_list_from_state_dict(sd, root, batchnorm, use_bias):
    """model.get_weights() order of the Keras CNN whose transplant is `sd` (tests/test_gpu_net.py)"""
    out = []
    for kind, key in common.plain_module_order(root, batchnorm):
        if kind == "conv":
            out += [np.transpose(np.asarray(sd[key + ".weight"]), (2, 3, 1, 0)), np.asarray(sd[key + ".bias"])]
        elif kind == "bn":
            out += [np.asarray(sd[key + "." + n]) for n in ("weight", "bias", "running_mean", "running_var")]
        else:
            out.append(np.transpose(np.asarray(sd[key + ".weight"])))
            if use_bias:
                out.append(np.asarray(sd[key + ".bias"]))
    return out


def _session(tmp_path, monkeypatch, sess_id, root, C, pools):
    """<sess_id>.h5 (a placeholder; the weight list comes from an .npz behind keras_h5_weight_list: h5py is not installed),
    .mat and, with `pools`, .json -- as the session directories under MODEL_ROOT hold them"""
    import scipy.io

    from wsscam import synth

    mdir = tmp_path / sess_id
    os.makedirs(mdir)
    use_bias = root == "m7"
    sd = synth.plain_state_dict(root, C, True, seed=5)
    np.savez(str(mdir / (sess_id + ".npz")), *_keras_list_from_state_dict(sd, root, True, use_bias))
    (mdir / (sess_id + ".h5")).write_bytes(b"placeholder")
    scipy.io.savemat(str(mdir / (sess_id + ".mat")), {"optimalScoreThresh": np.full((1, C), 0.4)})
    if pools is not None:
        doc = kref.keras_document(kref.keras_layers(root, pools, True, use_bias, C), "dict")
        (mdir / (sess_id + ".json")).write_text(json.dumps(doc))

    def fake_h5(path):
        z = np.load(path[:-3] + ".npz")
        return [z["arr_%d" % i] for i in range(len(z.files))]

    monkeypatch.setattr(common, "keras_h5_weight_list", fake_h5)
    return str(mdir), sd


def test_load_model_reads_the_architecture_file(tmp_path, monkeypatch):
    from wsscam import keras_store
    from wsscam.cues import utilities as cues

    C = 7
    mdir, sd = _session(tmp_path, monkeypatch, "DeepGlobe_M7", "m7", C, SAME3)
    model, alpha, final_layer, thr = keras_store.load_model(mdir, "DeepGlobe_M7", "M7", "DeepGlobe")
    assert model.pooling == SAME3 and model.cam_size(224) == 56 and thr.shape == (1, C)
    assert np.array_equal(alpha, cues.get_grad_cam_weights(model, final_layer, np.zeros((1, 224, 224, 3))))
    want = common.grad_cam_alpha(sd["m7.classifier.0.weight"], 56, 56, "max", bn_scale=common.last_bn_affine(sd, "m7")[0])
    assert np.array_equal(alpha, want)
    # an odd input: the spec's map, not the halved one, on the device too
    assert model.cam_size(225) == 57 and 225 // 4 == 56
    # a VGG16 session at 321: the seed size of the rest of the pipeline (the 321 x 321 stack itself is not run here)
    vdir, _ = _session(tmp_path, monkeypatch, "VOC2012_VGG16", "vgg16", C, SAME3)
    model, alpha, _, _ = keras_store.load_model(vdir, "VOC2012_VGG16", "VGG16", "VOC2012")
    assert model.pooling == SAME3 and model.cam_size(321) == 41 and alpha.shape == (1024, C)
    os.remove(os.path.join(vdir, "VOC2012_VGG16.json"))
    model, _, _, _ = keras_store.load_model(vdir, "VOC2012_VGG16", "VGG16", "VOC2012")
    assert model.pooling is None and model.cam_size(321) == 40
    # an architecture file that contradicts the model type's BatchNorm flag is an error, not a choice
    doc = kref.keras_document(kref.keras_layers("vgg16", SAME3, False, False, C))
    with open(os.path.join(vdir, "VOC2012_VGG16.json"), "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError):
        keras_store.load_model(vdir, "VOC2012_VGG16", "VGG16", "VOC2012")
