"""GPU: wsc_cue_seeds / wsc_cue_maps (csrc/cue_seeds.hip), cues.utilities.seed_label_maps and gen_cues(device_seeds=True)
against the numpy oracle of tests/cue_seeds_ref.py.  Labels and areas are integers and the resized maps are held to the bits of
the existing chain, so every comparison is np.array_equal."""
import pickle

import numpy as np
import pytest

from tests import cue_seeds_ref as ref
from wsscam import _lib
from wsscam.cues import utilities as cues

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.2, 0.55)


def _seeds(ctx, fg, bg, thresh, per_image_max=False, bg_fraction=ref.BG_FRACTION, want_area=True):
    """The raw entry point: -> (labels uint8 (B, H, W), areas int32 (B, L) or None); output buffers pre-filled with 0xff, inputs
    checked to be untouched."""
    B, C, H, W = fg.shape
    L = C + (bg is not None)
    fg_dev = ctx.to_device(fg)
    bg_dev = None if bg is None else ctx.to_device(bg)
    lab_dev, area_dev = ctx.alloc(B * H * W), ctx.alloc(B * L * 4) if want_area else None
    _lib.check(ctx._lib.wsc_memset(ctx.h, lab_dev.ptr, 0xff, B * H * W))  # every cell must be written
    if want_area:
        _lib.check(ctx._lib.wsc_memset(ctx.h, area_dev.ptr, 0xff, B * L * 4))
    _lib.cue_seeds(ctx, fg_dev, bg_dev, B, C, 0 if bg is None else bg.shape[1], H, W, thresh, lab_dev, area_dev,
                   per_image_max=per_image_max, bg_fraction=bg_fraction)
    lab = ctx.to_host(lab_dev, (B, H, W), np.uint8)
    area = ctx.to_host(area_dev, (B, L), np.int32) if want_area else None
    assert np.array_equal(ctx.to_host(fg_dev, fg.shape, np.float32), fg)
    assert bg is None or np.array_equal(ctx.to_host(bg_dev, bg.shape, np.float32), bg)
    return lab, area


@pytest.fixture(scope="module")
def sweep():
    return ref.sweep_cases()


@pytest.mark.parametrize("idx", range(len(ref.SWEEP)), ids=[s[0] for s in ref.SWEEP])
def test_seeds_equal_oracle(ctx, sweep, idx):
    name, fg, bg = sweep[idx]
    for per_image in (False, True):
        for thresh in THRESHOLDS:
            want_lab, want_area, _ = ref.seeds(fg, bg, thresh, per_image_max=per_image)
            lab, area = _seeds(ctx, fg, bg, thresh, per_image_max=per_image)
            assert np.array_equal(area, want_area), (name, per_image, thresh)
            assert np.array_equal(lab, want_lab), (name, per_image, thresh)
    assert np.array_equal(_seeds(ctx, fg, bg, 0.2, want_area=False)[0], ref.seeds(fg, bg, 0.2)[0])  # area_dev = NULL


@pytest.mark.parametrize("case", ref.handmade_cases(), ids=lambda c: c[0])
def test_handmade_cases(ctx, case):
    """cue_seeds_ref.handmade_cases asserts, while it builds them, the properties of the inputs that the cases stand for."""
    name, fg, bg, kw, expect = case
    want_lab, want_area, _ = ref.seeds(fg, bg, **kw)
    lab, area = _seeds(ctx, fg, bg, kw["thresh"], kw.get("per_image_max", False), kw.get("bg_fraction", ref.BG_FRACTION))
    assert np.array_equal(lab, want_lab) and np.array_equal(area, want_area), name
    if expect is not None:
        assert np.array_equal(lab, expect), name


def _maps_by_chain(ctx, cams, chan, gate, S):
    """The existing chain: gate on the host in float64, transpose NHWC -> NCHW, wsc_bilinear_resize."""
    x = cams[:, :, :, chan].astype(np.float64)
    if gate is not None:
        x = x * gate[:, None, None, :]
    return cues.resize_stack(np.transpose(x, (0, 3, 1, 2)), (S, S), ctx=ctx).astype(np.float32)


@pytest.mark.parametrize("h,w,S", [(7, 9, 41), (56, 56, 41), (41, 41, 41)], ids=["7x9-up", "56-down", "41-identity"])
def test_cue_maps_bits(ctx, h, w, S):
    rng = np.random.default_rng(h * 100 + w)
    B, C_all = 3, 11
    cams = rng.normal(0.2, 1.0, (B, h, w, C_all)).astype(np.float32)  # both signs: a gated negative value is -0
    cams_dev = ctx.to_device(cams)
    for chan in (np.arange(C_all), np.array([9, 2, 3, 0, 6])):  # all channels; dropped and reordered
        gate = (rng.random((B, len(chan))) < 0.6).astype(np.float32)
        for g in (gate, None):
            out_dev = ctx.alloc(B * len(chan) * S * S * 4)
            _lib.check(ctx._lib.wsc_memset(ctx.h, out_dev.ptr, 0xff, B * len(chan) * S * S * 4))
            _lib.cue_maps(ctx, cams_dev, B, h, w, C_all, chan, None if g is None else ctx.to_device(g), S, out_dev)
            out = ctx.to_host(out_dev, (B, len(chan), S, S), np.float32)
            want = _maps_by_chain(ctx, cams, chan, g, S)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (h, w, S, len(chan), g is None)
    assert np.array_equal(ctx.to_host(cams_dev, cams.shape, np.float32), cams)
    if h == w == S:
        out_dev = ctx.alloc(cams.size * 4)
        _lib.cue_maps(ctx, cams_dev, B, h, w, C_all, np.arange(C_all), None, S, out_dev)
        assert np.array_equal(ctx.to_host(out_dev, (B, C_all, S, S), np.float32), np.transpose(cams, (0, 3, 1, 2)))


def test_limits(ctx):
    buf = ctx.alloc(1 << 20)

    def seeds(B, C, Cb, H, W, fg=buf, bg=buf, lab=buf, fraction=0.1):
        _lib.cue_seeds(ctx, fg, bg, B, C, Cb, H, W, 0.2, lab, None, bg_fraction=fraction)

    for kw, word in ((dict(B=1, C=32, Cb=1, H=8, W=8), "L=33"), (dict(B=1, C=33, Cb=0, H=8, W=8, bg=None), "L=33"),
                     (dict(B=1, C=0, Cb=1, H=8, W=8), "C=0"), (dict(B=1, C=2, Cb=0, H=8, W=8), "Cb=0"),
                     (dict(B=0, C=2, Cb=1, H=8, W=8), "B=0"), (dict(B=1, C=2, Cb=1, H=0, W=8), "H=0"),
                     (dict(B=1, C=2, Cb=1, H=8, W=-3), "W=-3"), (dict(B=1, C=2, Cb=1, H=1, W=4097), "4097 pixels"),
                     (dict(B=1, C=2, Cb=1, H=65, W=64), "4160 pixels"), (dict(B=1, C=2, Cb=1, H=8, W=8, fraction=1.0), "bg_fraction=1"),
                     (dict(B=1, C=2, Cb=1, H=8, W=8, fraction=-0.25), "bg_fraction=-0.25")):
        with pytest.raises(_lib.WscError) as ei:
            seeds(**kw)
        assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (kw, str(ei.value))
    for null in ("fg", "lab"):
        with pytest.raises(_lib.WscError) as ei:
            seeds(1, 2, 1, 8, 8, **{null: None})
        assert ei.value.status == _lib.WSC_ERR_INVALID

    def maps(B, h, w, C_all, chan, S, cams=buf, out=buf):
        _lib.cue_maps(ctx, cams, B, h, w, C_all, chan, None, S, out)

    for args, word in (((0, 4, 4, 3, [0], 5), "B=0"), ((1, 0, 4, 3, [0], 5), "h=0"), ((1, 4, -1, 3, [0], 5), "w=-1"),
                       ((1, 4, 4, 0, [0], 5), "C_all=0"), ((1, 4, 4, 3, [], 5), "C=0"), ((1, 4, 4, 3, [0], 0), "S=0"),
                       ((1, 4, 4, 3, [0, 3], 5), "chan[1]=3"), ((1, 4, 4, 3, [-1], 5), "chan[0]=-1")):
        with pytest.raises(_lib.WscError) as ei:
            maps(*args)
        assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (args, str(ei.value))
    for null in ("cams", "out"):
        with pytest.raises(_lib.WscError) as ei:
            maps(1, 4, 4, 3, [0], 5, **{null: None})
        assert ei.value.status == _lib.WSC_ERR_INVALID
    # the largest legal call: 64 x 64 pixels, L = 32 (31 classes + background)
    rng = np.random.default_rng(64)
    fg, bg = ref._stack(rng, 2, 31, 64, 64), ref._stack(rng, 2, 3, 64, 64)
    fg[:, 30] = 0
    fg[:, 30, 62:, 62:] = 1  # the last channel holds the smallest mask: bit 31 of the last pixels' words, label 32
    want_lab, want_area, _ = ref.seeds(fg, bg, 0.2)
    assert (want_lab[:, 62:, 62:] == 32).all() and (want_area[:, 31] == 4).all()
    lab, area = _seeds(ctx, fg, bg, 0.2)
    assert np.array_equal(lab, want_lab) and np.array_equal(area, want_area)


def test_seed_label_maps(ctx, sweep):
    name, fg, bg = sweep[0]
    want_lab, want_area, _ = ref.seeds(fg, bg, 0.2)
    fg_in, bg_in = fg.astype(np.float64), bg.astype(np.float64)  # float64 that float32 holds exactly: accepted
    lab, area = cues.seed_label_maps(fg_in, bg_in, 0.2, ctx=ctx)
    assert lab.dtype == np.uint8 and area.dtype == np.int32 and np.array_equal(lab, want_lab) and np.array_equal(area, want_area)
    assert np.array_equal(fg_in, fg) and np.array_equal(bg_in, bg)
    lab, area = cues.seed_label_maps(fg, None, 0.2, per_image_max=True, ctx=ctx)
    want = ref.seeds(fg, None, 0.2, per_image_max=True)
    assert np.array_equal(lab, want[0]) and np.array_equal(area, want[1])
    off = fg_in.copy()
    off[0, 0, 0, 0] = 0.1  # not a float32
    with pytest.raises(ValueError):
        cues.seed_label_maps(off, bg_in, 0.2, ctx=ctx)
    with pytest.raises(ValueError):
        cues.seed_label_maps(fg_in, bg_in + 1e-12, 0.2, ctx=ctx)


def _check_driver(gen, ctx_of, models, alphas, thr, norm_batches, labels_keep, keep_inds, thresh, is_voc, out_dir, n_images):
    """gen(device_seeds) -> cue dict.  The device result equals the oracle applied to the maps the host path forms, exactly; it
    equals the host result on every non-ambiguous pixel; labels identical; cue arrays int64 (3, n)."""
    host = gen(False)
    dev = gen(True)
    name = "localization_cues.pickle"
    with open(out_dir / name, "rb") as f:
        saved = pickle.load(f)
    assert sorted(saved) == sorted(dev) == sorted(host)
    for k in dev:
        assert np.array_equal(np.asarray(saved[k]), np.asarray(dev[k])), k
    checked = 0
    for (lo, hi), norm in norm_batches:
        H = {}
        for m in models:
            cams, scores = cues.conv_and_cams(models[m], np.asarray(alphas[m]), norm, relu=True, want_scores=True)
            ip = np.greater_equal(scores[:, keep_inds], thr[m]) * labels_keep[lo:hi]
            cams = cams[:, :, :, keep_inds].astype(np.float64) * ip[:, None, None, :]
            H[m] = cues.resize_stack(np.transpose(cams, (0, 3, 1, 2)), (41, 41), ctx=ctx_of(m))
        want_lab, _, amb = ref.seeds(H["fg"].astype(np.float32), H["bg"].astype(np.float32) if is_voc else None, thresh)
        idx = list(range(lo, hi))
        want = cues.cues_from_label_maps({}, want_lab, [None] * len(idx), idx)
        got_lab = ref.labels_from_cues(dev, idx, 41, 41)
        host_lab = ref.labels_from_cues(host, idx, 41, 41)
        assert np.array_equal(got_lab, want_lab)
        assert np.array_equal(got_lab[~amb], host_lab[~amb])
        for i in idx:
            a = dev["%d_cues" % i]
            assert a.dtype == np.int64 and a.ndim == 2 and a.shape[0] == 3
            assert np.array_equal(a, want["%d_cues" % i])
            assert np.array_equal(dev["%d_labels" % i], host["%d_labels" % i])
            checked += a.shape[1]
    assert checked > 0 and hi == n_images


def test_gen_cues_device_seeds_voc(tmp_path):
    """VOC2012 / VGG16, fg + bg models: models, images and thresholds of tests/test_gpu_net.py::test_gen_cues_driver."""
    from oracle import cnn_ref
    from tests.test_gpu_net import _vgg_model
    from wsscam.cues import demo as cues_demo

    C = 20
    fg, sd_fg = _vgg_model(C, seed=8)
    bg, sd_bg = _vgg_model(C, seed=9)
    rng = np.random.default_rng(10)
    images = [cnn_ref.synth_image(rng, 300, 340), cnn_ref.synth_image(rng, 375, 500), cnn_ref.synth_image(rng, 321, 321)]
    labels = (rng.random((3, C)) < 0.2).astype(np.float64)
    labels[:, 3] = 1
    alphas = {"fg": cnn_ref.grad_cam_weights(sd_fg, "vgg16", cnn_ref.VGG16_CFG, 33, C),
              "bg": cnn_ref.grad_cam_weights(sd_bg, "vgg16", cnn_ref.VGG16_CFG, 33, C)}
    thr = {"fg": np.full((1, C), 0.45), "bg": np.full((1, C), 0.45)}
    models = {"fg": fg, "bg": bg}

    def gen(device_seeds):
        return cues_demo.gen_cues("VOC2012", "VGG16", 0.2, 2, models=models, alphas=alphas, thresholds=thr, images=images,
                                  labels=labels, out_dir=str(tmp_path), is_verbose=False, device_seeds=device_seeds)

    batches = [((lo, hi), cues_demo.read_batch(images[lo:hi], (321, 321), [104, 117, 123], [255, 255, 255], ctx=fg.ctx)[0])
               for lo, hi in ((0, 2), (2, 3))]
    _check_driver(gen, lambda m: models[m].ctx, models, alphas, thr, batches, labels, np.arange(C), 0.2, True, tmp_path, 3)


def test_gen_cues_device_seeds_deepglobe(tmp_path):
    """DeepGlobe / M7, the fg-only path with ignore_ind: model, images and thresholds of
    tests/test_gpu_net.py::test_gen_cues_reference_call_form (its explicit-objects call)."""
    from oracle import cnn_ref
    from wsscam import synth
    from wsscam.cues import demo as cues_demo
    from wsscam.net import m7_cam

    C = 7
    rng = np.random.default_rng(21)
    images = [cnn_ref.synth_image(rng, 224, 224) for _ in range(3)]
    labels = (rng.random((3, C)) < 0.4).astype(np.float32)
    labels[:, 1] = 1
    sd = synth.plain_state_dict("m7", C, True, seed=5)
    thr = np.full((1, C), 0.4)
    model = m7_cam.CAM(None, "deepglobe", "M7", C, None)
    model.load_state_dict(dict(sd))
    model.cuda(0)
    alpha = cues.get_grad_cam_weights(model, cues.find_final_layer(model), np.zeros((1, 224, 224, 3)))
    keep = np.delete(np.arange(C), 6)
    models, alphas = {"fg": model}, {"fg": alpha}

    def gen(device_seeds):
        return cues_demo.gen_cues("DeepGlobe", "M7", 0.2, 2, is_verbose=False, models=models, alphas=alphas,
                                  thresholds={"fg": thr}, images=images, labels=labels, out_dir=str(tmp_path),
                                  device_seeds=device_seeds)

    batches = [((lo, hi), cues_demo.read_batch(images[lo:hi], (224, 224), [0, 0, 0], [255, 255, 255], ctx=model.ctx)[0])
               for lo, hi in ((0, 2), (2, 3))]
    _check_driver(gen, lambda m: model.ctx, models, alphas, {"fg": thr[:, keep]}, batches, labels[:, keep], keep, 0.2, False,
                  tmp_path, 3)
