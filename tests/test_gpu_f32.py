"""GPU: the exact-fp32 mode (PREC_F32): fp32 weights and activations on the fp32-input MFMA (csrc/conv_f32.hip), the mode
WSC_ERR_RANGE sends a saturating checkpoint to.

Single layers are held to a DERIVED bound, not a measured one: every output is a length-K fp32 fma chain (K = Cin kh kw) plus
the epilogue's roundings, so |y - ref64| <= (K + 8) 2^-24 A with A = conv(|x|, |w|) |scale| + |shift| + |residual| in float64.
Networks are held to the project's bounds for its fp32-class mode f16x3 (tests/test_gpu_net.py, tests/test_gpu_irn.py): the
exact mode meets the bar of the mode it stands in for.  Shape lists, builders and measures are imported from those files."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cnn_ref, irn_ref
from tests import test_gpu_conv, test_gpu_irn, test_gpu_net, test_gpu_range
from wsscam import _lib
from wsscam.net import m7_cam, m7_irn, resnet50_cam, resnet50_irn, vgg16_cam, vgg16_irn

pytestmark = pytest.mark.gpu

P = getattr(_lib, "PREC_F32", 4)  # (without the feature: "unknown precision 4" from the first call)
F16X3 = _lib.PREC_F16X3
U = 2.0 ** -24  # unit round-off of fp32


def _draw_layer(shape):
    """operands exactly as tests/test_gpu_conv.py::test_conv_layer draws them"""
    N, Cin, H, W, Cout, k, stride, pad = shape
    rng = np.random.default_rng(abs(hash(shape)) % (2 ** 31))
    x = rng.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k))).astype(np.float32)
    w *= (1.0 + 0.5 * np.arange(Cout, dtype=np.float32) / Cout)[:, None, None, None]
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = rng.normal(0, 1, (N, Cout, Ho, Wo)).astype(np.float32)
    return x, w, scale, shift, res


@pytest.mark.parametrize("shape", test_gpu_conv.SHAPES)
def test_conv_layer_f32_rounding_error_bound(ctx, shape):
    N, Cin, H, W, Cout, k, stride, pad = shape
    x, w, scale, shift, res = _draw_layer(shape)
    K = Cin * k * k
    t = lambda a: torch.from_numpy(a).double()
    per_c = lambda v: t(v)[None, :, None, None]
    conv = F.conv2d(t(x), t(w), stride=stride, padding=pad)
    conv_abs = F.conv2d(t(x).abs(), t(w).abs(), stride=stride, padding=pad)
    for use_res, relu in ((False, False), (True, True)):
        y = test_gpu_conv._run(ctx, x, w, stride, pad, scale, shift, res if use_res else None, relu, P)
        ref = conv * per_c(scale) + per_c(shift)
        A = conv_abs * per_c(scale).abs() + per_c(shift).abs()
        if use_res:
            ref = ref + t(res)
            A = A + t(res).abs()
        if relu:
            ref = torch.relu(ref)
        ref, A = ref.numpy(), A.numpy()
        assert y.shape == ref.shape and y.dtype == np.float32
        err = np.abs(y.astype(np.float64) - ref)
        print("f32 conv %s res/relu=%d: K = %d, max |y - ref64| / (2^-24 A) = %.2f (bound %d)" % (shape, use_res, K, (err / (U * A)).max(), K + 8))
        bad = err > (K + 8) * U * A
        assert not bad.any(), "shape %s res %s: %d beyond the fma-chain bound, worst %.3g x 2^-24 A at %s" % (
            shape, use_res, bad.sum(), (err / (U * A)).max(), np.unravel_index((err / A).argmax(), err.shape))
        # WSC_CONV_GENERIC has nothing to select in this mode: accepted, same bits
        y_g = test_gpu_conv._run(ctx, x, w, stride, pad, scale, shift, res if use_res else None, relu, P | _lib.CONV_GENERIC)
        assert np.array_equal(y, y_g)


@pytest.mark.parametrize("shape", [(4, 3, 33, 37, 64, 7, 2, 3), (4, 3, 21, 23, 128, 3, 1, 1), (4, 128, 21, 21, 128, 3, 2, 1),
                                   (4, 256, 9, 11, 72, 1, 1, 0)])
def test_conv_layer_f32_repeatable_and_batch_independent(ctx, shape):
    """No tolerance: the same layer twice, and N = 4 against its four N = 1 runs (a fixed K order, no atomics, no split-K)."""
    N, Cin, H, W, Cout, k, stride, pad = shape
    x, w, scale, shift, res = _draw_layer(shape)
    y = test_gpu_conv._run(ctx, x, w, stride, pad, scale, shift, res, True, P)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    assert np.array_equal(y, test_gpu_conv._run(ctx, x, w, stride, pad, scale, shift, res, True, P))
    for n in range(N):
        y1 = test_gpu_conv._run(ctx, x[n:n + 1], w, stride, pad, scale, shift, res[n:n + 1], True, P)
        assert np.array_equal(y1[0], y[n]), (shape, n)


# ---- networks: the f16x3 bounds of tests/test_gpu_net.py / tests/test_gpu_irn.py ---------------------------------------
@pytest.mark.parametrize("S", [64, 97])
def test_resnet50_cam_f32_vs_golden(golden, S):
    sd = cnn_ref.make_resnet50_cam_state_dict(20, seed=0)
    model = test_gpu_net._model(resnet50_cam.CAM, sd, 20, P)
    cam = model.forward(golden["x_S%d" % S])
    ref = golden["cam_S%d" % S]
    assert cam.shape == ref.shape
    d = np.abs(cam - ref).max() / ref.max()
    print("resnet50_cam f32 S=%d: raw %.2e x max" % (S, d))
    assert d <= test_gpu_net.TOL_RAW[F16X3] == 2e-5, d
    assert model.ctx.range_status() == 0


def test_resnet50_make_cam_321_f32(golden):
    """the 3-image 321 x 321 make_cam batch of tests/test_gpu_net.py::test_resnet50_make_cam_321"""
    from wsscam.step import make_cam

    sd = cnn_ref.make_resnet50_cam_state_dict(20, seed=0)
    model = test_gpu_net._model(resnet50_cam.CAM, sd, 20, P)
    rng = np.random.default_rng(3)
    sizes = [(375, 500), (500, 333), (281, 500)]
    imgs = [golden["img_321"]] + [cnn_ref.synth_image(rng, h, w) for (h, w) in sizes[1:]]
    labels = [np.zeros(20, np.float32) for _ in sizes]
    labels[0][[3, 11]] = 1
    labels[1][[0]] = 1
    labels[2][[5, 7, 19]] = 1
    packs = [{"name": "img%d" % i, "img": cnn_ref.msf_pack(im, (321, 321)), "size": sz, "label": lb}
             for i, (im, sz, lb) in enumerate(zip(imgs, sizes, labels))]

    class Args:
        split = "train_aug"
        dataset = "voc12"
        cam_out_dir = None

    outs = make_cam.process_batch(model, packs, Args, save=False)
    for p, o in zip(packs, outs):
        ref = cnn_ref.make_cam_image(torch.from_numpy(p["img"]), sd, p["size"], torch.from_numpy(p["label"]))
        assert np.array_equal(o["keys"], ref["keys"])
        assert o["cam"].shape == ref["cam"].shape and o["high_res"].shape == ref["high_res"].shape
        d1 = np.abs(o["cam"] - ref["cam"]).max()
        d2 = np.abs(o["high_res"] - ref["high_res"]).max()
        print("make_cam 321 f32 %s: normalised %.2e / %.2e" % (p["name"], d1, d2))
        assert d1 <= test_gpu_net.TOL_NORM[F16X3] == 1e-4 and d2 <= 1e-4, (d1, d2)
        if len(ref["keys"]) > 1:
            agree = (o["high_res"].argmax(0) == ref["high_res"].argmax(0)).mean()
            assert agree >= 0.9999, agree


@pytest.mark.parametrize("batchnorm", [True, False])
def test_vgg16_cam_f32(batchnorm):
    C = 20
    sd = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, batchnorm, seed=1)
    model = test_gpu_net._model(vgg16_cam.CAM, sd, C, P)
    rng = np.random.default_rng(4)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(rng, 80, 90), (65, 65))
    cam, score = model.forward_batch(x[None], want_score=True)
    with torch.no_grad():
        rcam, rscore = cnn_ref.vgg16_cam_forward(torch.from_numpy(x), sd, C)
    assert cam[0].shape == tuple(rcam.shape) == (C, 8, 8)
    d, ds = np.abs(cam[0] - rcam.numpy()).max() / float(rcam.max()), np.abs(score[0] - rscore.numpy()).max()
    print("vgg16_cam f32 bn=%s: raw %.2e x max, scores %.2e" % (batchnorm, d, ds))
    assert d <= test_gpu_net.TOL_RAW[F16X3]
    assert ds <= 2e-5


def test_m7_cam_f32():
    C, tol = 20, 1e-4  # (test_m7_cam's f16x3 bound)
    sd = cnn_ref.make_plain_state_dict("m7", cnn_ref.M7_CFG, C, True, seed=2)
    alpha = cnn_ref.grad_cam_weights(sd, "m7", cnn_ref.M7_CFG, 32, C)
    sd_dev = dict(sd)
    sd_dev["gradcam_weights"] = torch.from_numpy(alpha.astype(np.float32))
    model = test_gpu_net._model(m7_cam.CAM, sd_dev, C, P)
    rng = np.random.default_rng(5)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(rng, 70, 60), (64, 64))
    cam, score = model.forward_batch(x[None], want_score=True)
    with torch.no_grad():
        rcam, rscore = cnn_ref.m7_cam_forward(torch.from_numpy(x), sd, torch.from_numpy(alpha), C)
    assert cam[0].shape == tuple(rcam.shape) == (C, 16, 16)
    d, ds = np.abs(cam[0] - rcam.numpy()).max() / max(float(rcam.max()), 1e-3), np.abs(score[0] - rscore.numpy()).max()
    print("m7_cam f32: raw %.2e x max, scores %.2e" % (d, ds))
    assert d <= tol and ds <= tol


def test_resnet50_irn_f32_vs_reference_fixture():
    g = np.load(test_gpu_irn.GOLDEN)
    sd = irn_ref.make_resnet50_irn_state_dict(seed=int(g["seed"]))
    m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=int(g["crop_size"]), stride=int(g["stride"]), precision=P)
    m.load_state_dict(sd)
    m.eval().cuda(0)
    edge, dp = m.forward(g["x"])
    assert edge.shape == g["edge"].shape and dp.shape == g["dp"].shape
    te, td = test_gpu_irn.TOL[F16X3]
    de, dd = np.abs(edge - g["edge"]).max(), np.abs(dp - g["dp"]).max()
    print("resnet50_irn f32: edge %.2e, dp %.2e (max |dp| %.3g)" % (de, dd, np.abs(g["dp"]).max()))
    assert de <= te and dd <= td * max(1.0, float(np.abs(g["dp"]).max()))


@pytest.mark.parametrize("batchnorm", [True, False])
def test_vgg16_irn_f32_vs_oracle(batchnorm):
    sd = irn_ref.make_vgg16_irn_state_dict(seed=2, batchnorm=batchnorm)
    m = vgg16_irn.EdgeDisplacement(None, "voc12" if batchnorm else "adp_morph", "", 20, None, crop_size=96, stride=4, precision=P)
    m.load_state_dict(sd)
    m.eval().cuda(0)
    rng = np.random.default_rng(3)
    xs = np.stack([cnn_ref.msf_pack(cnn_ref.synth_image(rng, 77, 90), (77, 90)) for _ in range(2)])
    edge, dp = m.forward_batch(xs)
    for b in range(2):
        with torch.no_grad():
            e, d = irn_ref.edge_displacement_forward(torch.from_numpy(xs[b]), sd, "vgg16", crop_size=96, stride=4)
        assert edge[b].shape == tuple(e.shape) == (1, 20, 23) and dp[b].shape == tuple(d.shape)
        de, dd = np.abs(edge[b] - e.numpy()).max(), np.abs(dp[b] - d.numpy()).max()
        print("vgg16_irn f32 bn=%s image %d: edge %.2e, dp %.2e" % (batchnorm, b, de, dd))
        assert de <= 2e-4 and dd <= 2e-3 * max(1.0, float(d.abs().max()))  # (test_vgg16_irn_vs_oracle's bounds)


def test_m7_irn_f32_vs_oracle():
    sd = irn_ref.make_m7_irn_state_dict(seed=4)
    m = m7_irn.EdgeDisplacement(None, "voc12", "", 20, None, crop_size=64, stride=4, precision=P)
    m.load_state_dict(sd)
    m.eval().cuda(0)
    rng = np.random.default_rng(6)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(rng, 52, 61), (52, 61))
    edge, dp = m.forward(x)
    with torch.no_grad():
        e, d = irn_ref.edge_displacement_forward(torch.from_numpy(x), sd, "m7", crop_size=64, stride=4)
    assert edge.shape == tuple(e.shape) == (1, 13, 16) and dp.shape == tuple(d.shape) == (2, 13, 16)
    assert np.abs(edge - e.numpy()).max() <= 2e-4 and np.abs(dp - d.numpy()).max() <= 2e-3 * max(1.0, float(d.abs().max()))


# ---- the case the mode exists for: the two networks of tests/test_gpu_range.py::test_f16x3_overflow_fails_loudly ------------
def _overflow_case(arch):
    C, S = 20, 65
    rng = np.random.default_rng(13)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(rng, 90, 70), (S, S))
    if arch == "resnet50":
        sd = test_gpu_range._resnet_large_stage(cnn_ref.make_resnet50_cam_state_dict(C, seed=3), 16)
        return C, x, sd, resnet50_cam.CAM
    sd = dict(cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, False, seed=6))
    first = "vgg16.%s.0" % cnn_ref.VGG16_CFG[0][0]
    sd[first + ".weight"] = sd[first + ".weight"] * 2.0 ** 18
    sd[first + ".bias"] = sd[first + ".bias"] * 2.0 ** 18
    return C, x, sd, vgg16_cam.CAM


def _two_measures(cam, ref):
    """test_gpu_range._check_cam's raw and normalised measures, as numbers"""
    raw = np.abs(cam - ref).max() / ref.max()
    nrm = lambda c: c / (c.max(axis=(1, 2), keepdims=True) + 1e-5 * ref.max())
    return raw, np.abs(nrm(cam) - nrm(ref)).max()


@pytest.mark.parametrize("arch", ["resnet50", "vgg16_nobn"])
def test_f32_computes_what_saturates_the_half_modes(arch):
    """A network that raises WSC_ERR_RANGE in f16x3 returns the reference's maps in PREC_F32: against a float64 evaluation
    of the same state dict, raw <= 2e-5 x max and normalised <= 1e-4 (VGG16 scores <= 2e-5)."""
    C, x, sd, cls = _overflow_case(arch)
    model = test_gpu_net._model(cls, sd, C, P)
    if arch == "resnet50":
        cam, score = model.forward(x), None
    else:
        cams, scores = model.forward_batch(x[None], want_score=True)
        cam, score = cams[0], scores[0]
    model.ctx.sync()  # does not raise
    assert model.ctx.range_status() == 0
    sd64 = {k: v.double() for k, v in sd.items()}
    x64 = torch.from_numpy(x).double()
    with torch.no_grad():
        if arch == "resnet50":
            ref64 = cnn_ref.resnet50_cam_forward(x64, sd64)
            ref32, s64, s32 = cnn_ref.resnet50_cam_forward(torch.from_numpy(x), sd), None, None
        else:
            ref64, s64 = cnn_ref.vgg16_cam_forward(x64, sd64, C)
            ref32, s32 = cnn_ref.vgg16_cam_forward(torch.from_numpy(x), sd, C)
    ref64 = ref64.numpy()
    assert np.isfinite(cam).all() and float(ref64.max()) > 0
    raw, nrm = _two_measures(cam.astype(np.float64), ref64)
    raw_o, nrm_o = _two_measures(ref32.numpy().astype(np.float64), ref64)
    print("%s past the half ceiling, against float64: device f32 raw %.2e / normalised %.2e; torch fp32 oracle %.2e / %.2e" % (
        arch, raw, nrm, raw_o, nrm_o))
    if score is not None:
        ds, ds_o = np.abs(score - s64.numpy()).max(), np.abs(s32.numpy() - s64.numpy()).max()
        print("%s scores against float64: device %.2e, torch fp32 oracle %.2e" % (arch, ds, ds_o))
    assert raw <= 2e-5, raw
    assert nrm <= 1e-4, nrm
    if score is not None:
        assert ds <= 2e-5, ds


def test_f32_power_of_two_invariance_is_bit_exact():
    """_resnet_large_stage moves powers of two between a BatchNorm and the convolutions behind it; absent overflow and
    underflow every fp32 operation commutes with that, so the maps of the k = 11 and k = 16 networks equal the k = 0 maps
    bit for bit -- no value-dependent path, no 16-bit intermediate anywhere in the mode."""
    C, S = 20, 65
    rng = np.random.default_rng(13)
    x = cnn_ref.msf_pack(cnn_ref.synth_image(rng, 90, 70), (S, S))
    base = cnn_ref.make_resnet50_cam_state_dict(C, seed=3)
    cams = {}
    for k in (0, 11, 16):
        cams[k] = test_gpu_net._model(resnet50_cam.CAM, test_gpu_range._resnet_large_stage(base, k), C, P).forward(x)
    assert np.isfinite(cams[0]).all() and cams[0].max() > 0
    for k in (11, 16):
        assert np.array_equal(cams[k], cams[0]), (k, np.abs(cams[k] - cams[0]).max())


def test_f32_batch_independent_and_repeatable():
    C, S, B = 20, 65, 3
    sd = cnn_ref.make_resnet50_cam_state_dict(C, seed=0)
    rng = np.random.default_rng(77)
    x = np.stack([cnn_ref.msf_pack(cnn_ref.synth_image(rng, 80 + 7 * b, 90 - 5 * b), (S, S)) for b in range(B)])
    m = test_gpu_net._model(resnet50_cam.CAM, sd, C, P)
    cam = m.forward_batch(x)
    assert cam.shape[:2] == (B, C) and np.isfinite(cam).all() and (cam >= 0).all() and cam.max() > 0
    for b in range(B):
        assert np.array_equal(m.forward_batch(x[b:b + 1])[0], cam[b]), b
    assert np.array_equal(m.forward_batch(x), cam)


def test_make_cam_run_f32_end_to_end(tmp_path):
    """step.make_cam.run with cam_precision=PREC_F32, set up as tests/test_gpu_edge.py::test_make_cam_run_end_to_end"""
    from wsscam.step import make_cam

    sd = cnn_ref.make_resnet50_cam_state_dict(20, seed=0)
    rng = np.random.default_rng(2)
    sizes = [(60, 80), (97, 64), (64, 64), (33, 47), (80, 60)]
    labels = [np.zeros(20, np.float32) for _ in sizes]
    labels[0][[1, 4]] = 1
    labels[1][[7]] = 1
    labels[3][[0, 19]] = 1
    labels[4][[12]] = 1
    data = [{"name": "2007_%06d" % i, "img": cnn_ref.msf_pack(cnn_ref.synth_image(rng, *sz), (65, 65)), "size": sz,
             "label": lb} for i, (sz, lb) in enumerate(zip(sizes, labels))]
    args = types.SimpleNamespace(cam_network="net.resnet50_cam", model_dir=None, dataset="voc12", tag="", num_classes=20,
                                 use_cls=None, model_id="resnet50", cam_weights_name=None, state_dict=sd,
                                 dataset_obj=data, split="train_aug", cam_out_dir=str(tmp_path), n_gpus=1,
                                 cam_batch_images=2, cam_precision=P)
    make_cam.run(args)
    assert sorted(os.listdir(tmp_path)) == [d["name"] + ".npy" for d in data]
    for d in data:
        rec = np.load(os.path.join(tmp_path, d["name"] + ".npy"), allow_pickle=True).item()
        ref = cnn_ref.make_cam_image(torch.from_numpy(d["img"]), sd, d["size"], torch.from_numpy(d["label"]))
        assert list(rec) == ["keys", "cam", "high_res"]
        if d["label"].sum() == 0:
            assert all(rec[k].shape == (0,) for k in rec)
            continue
        assert rec["keys"].dtype == np.int64 and np.array_equal(rec["keys"], ref["keys"])
        assert rec["cam"].shape == ref["cam"].shape and rec["high_res"].shape == ref["high_res"].shape
        assert np.abs(rec["high_res"] - ref["high_res"]).max() <= 1e-4
        assert np.abs(rec["cam"] - ref["cam"]).max() <= 1e-4
