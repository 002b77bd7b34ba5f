"""GPU: wsc_render_labels (csrc/render.hip) and the should_saveimg paths built on it against the numpy oracle of tests/render_ref.py.
Every comparison is on bytes: zero differing bytes, no tolerance.

The kernel cases are the smallest at which it can go wrong: a ragged batch of five images whose packed byte offsets (0, 5883,
6027, 6030, 6459) are on no 16-byte grid, with output rows of 53, 3, 1, 11 and 6 pixels -- rows shorter than the six pixels a
16-byte chunk touches, images smaller than one chunk (scalar path only), one- and two-stage nearest resizes and the pass-through."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import render_ref as ref
from tests import test_gpu_scratch as sweep
from wsscam import _lib, render

pytestmark = pytest.mark.gpu

# (label map, mid or None, output), all (height, width)
BATCH = [((41, 41), None, (37, 53)), ((5, 7), None, (16, 3)), ((1, 1), None, (1, 1)), ((7, 9), (20, 20), (13, 11)), ((6, 6), None, (6, 6))]
SRC, MID, OUT = [b[0] for b in BATCH], [b[1] for b in BATCH], [b[2] for b in BATCH]
OTHER = (9, 250, 77)
GUARD = 256
BAND = 0xA5
BLENDS = [("uint8", 0.75), ("uint8", 0.25), ("uint8", 0.3), ("float256", 0.75), ("float256", 0.25), ("float256", 0.3)]


@functools.lru_cache(maxsize=None)
def inputs(dtype_name, n_colours):
    """label maps with every kind of unlisted label among them, a palette, images at the output sizes"""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(100 + n_colours)
    special = [n_colours, 255] + ([-1, 2 ** 31 - 1, -2 ** 31, 256] if dtype == np.int32 else [])
    labels = []
    for h, w in SRC:
        lab = rng.integers(0, n_colours, (h, w)).astype(dtype)
        where = rng.random((h, w)) < 0.2
        lab[where] = rng.choice(np.array(special, dtype=np.int64), int(where.sum())).astype(dtype)
        labels.append(lab)
    labels[0][0, :len(special)] = np.array(special, dtype=np.int64).astype(dtype)  # (each of them at least once)
    palette = rng.integers(0, 256, (n_colours, 3)).astype(np.uint8)
    images = [rng.integers(0, 256, hw + (3,)).astype(np.uint8) for hw in OUT]
    return labels, palette, images


@functools.lru_cache(maxsize=None)
def expected(dtype_name, n_colours, rule, overlay_r):
    labels, palette, images = inputs(dtype_name, n_colours)
    return [ref.render(lab.astype(np.int64), palette, out, mid_hw=mid, other_rgb=OTHER, img=im, overlay_r=overlay_r, rule=rule)
            for lab, mid, out, im in zip(labels, MID, OUT, images)]


def run_kernel(ctx, dtype_name, n_colours, rule, overlay_r, with_overlay=True, shifts=(0, 0, 0)):
    """One launch on guarded buffers -> (colour bytes, overlay bytes or None, out_off); asserts the guard bands.  shifts: bytes
    by which the colour, overlay and image arrays are moved off hipMalloc's alignment."""
    labels, palette, images = inputs(dtype_name, n_colours)
    out_off = np.concatenate(([0], np.cumsum([3 * h * w for h, w in OUT]))).astype(np.int64)
    total = int(out_off[-1])
    lab_dev = ctx.to_device(np.concatenate([m.reshape(-1) for m in labels]))
    lab_off = np.concatenate(([0], np.cumsum([h * w for h, w in SRC])))[:-1]
    room = total + 2 * GUARD + 16
    bufs = [ctx.alloc(room) for _ in range(3)]
    for b in bufs:
        _lib.check(ctx._lib.wsc_memset(ctx.h, b.ptr, BAND, room))
    colour_p, overlay_p, img_p = (b.ptr + GUARD + s for b, s in zip(bufs, shifts))
    packed = np.concatenate([im.reshape(-1) for im in images])  # (held until the copy has returned)
    _lib.check(ctx._lib.wsc_memcpy_h2d(ctx.h, img_p, packed.ctypes.data, total))
    pal, other = render.palette_bytes(palette, OTHER, rule)
    _lib.render_labels(ctx, lab_dev, np.dtype(dtype_name), SRC, OUT, lab_off, out_off[:-1], pal, other, colour_p,
                       mid_sizes=[m or (0, 0) for m in MID], img_dev=img_p if with_overlay else None,
                       blend=render.blend_table(palette, OTHER, overlay_r, rule) if with_overlay else None,
                       overlay_dev=overlay_p if with_overlay else None)
    got = [ctx.to_host(b.ptr, (room,), np.uint8) for b in bufs[:2]]
    res = []
    for g, s, written in zip(got, shifts, (True, with_overlay)):
        lo = GUARD + s
        assert (g[:lo] == BAND).all() and (g[lo + total:] == BAND).all(), "a store outside the output"
        if not written:
            assert (g == BAND).all(), "overlay_dev = NULL, yet the second buffer was written"
        res.append(g[lo:lo + total] if written else None)
    return res[0], res[1], out_off


def compare(got, out_off, want, what):
    for b, w in enumerate(want):
        g = got[out_off[b]:out_off[b + 1]].reshape(w.shape)
        bad = g != w
        assert not bad.any(), "%s of image %d: %d of %d bytes differ, first at %s: %d vs %d" % (
            what, b, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), int(g[bad][0]), int(w[bad][0]))


@pytest.mark.parametrize("rule,overlay_r", BLENDS)
@pytest.mark.parametrize("n_colours", [1, 21, 63])
@pytest.mark.parametrize("dtype_name", ["uint8", "int32"])
def test_ragged_batch_against_the_oracle(ctx, dtype_name, n_colours, rule, overlay_r):
    colour, overlay, out_off = run_kernel(ctx, dtype_name, n_colours, rule, overlay_r)
    want = expected(dtype_name, n_colours, rule, overlay_r)
    compare(colour, out_off, [w[0] for w in want], "colour")
    compare(overlay, out_off, [w[1] for w in want], "overlay")


@pytest.mark.parametrize("n_colours", [1, 21, 63])
@pytest.mark.parametrize("dtype_name", ["uint8", "int32"])
def test_without_overlay_the_colour_image_is_the_same_and_nothing_else_is_written(ctx, dtype_name, n_colours):
    colour, overlay, out_off = run_kernel(ctx, dtype_name, n_colours, "uint8", 0.75, with_overlay=False)
    assert overlay is None
    compare(colour, out_off, [w[0] for w in expected(dtype_name, n_colours, "uint8", 0.75)], "colour")


@pytest.mark.parametrize("shifts", [(7, 7, 7), (5, 0, 3), (0, 1, 0)])
def test_arrays_off_the_16_byte_grid(ctx, shifts):
    """the three arrays on one grid that is not hipMalloc's (another head and tail), and on different grids (the scalar path)"""
    colour, overlay, out_off = run_kernel(ctx, "int32", 21, "uint8", 0.3, shifts=shifts)
    want = expected("int32", 21, "uint8", 0.3)
    compare(colour, out_off, [w[0] for w in want], "colour")
    compare(overlay, out_off, [w[1] for w in want], "overlay")


def test_render_labels_wrapper_returns_the_host_arrays(ctx):
    """wsscam.render.render_labels from host label maps and host images, both rules"""
    labels, palette, images = inputs("int32", 21)
    for rule, r in (("uint8", 0.75), ("float256", 0.25)):
        colours, overlays = render.render_labels(ctx, labels, SRC, OUT, palette, OTHER, mid_sizes=MID, images=images, overlay_r=r, rule=rule)
        for b, (wc, wo) in enumerate(expected("int32", 21, rule, r)):
            assert np.array_equal(colours[b], wc) and np.array_equal(overlays[b], wo), (rule, b)
    colours, overlays = render.render_labels(ctx, labels, SRC, OUT, palette, OTHER, mid_sizes=MID)
    assert overlays is None
    assert all(np.array_equal(c, w[0]) for c, w in zip(colours, expected("int32", 21, "uint8", 0.75)))


@sweep.case("render-labels", "wsc_render_labels")
def _render_labels(ctx):
    labels, palette, images = inputs("uint8", 63)
    colours, overlays = render.render_labels(ctx, labels, SRC, OUT, palette, OTHER, mid_sizes=MID, images=images, overlay_r=0.3)
    for (wc, wo), c, o in zip(expected("uint8", 63, "uint8", 0.3), colours, overlays):
        assert np.array_equal(c, wc) and np.array_equal(o, wo)
    return [np.concatenate([a.reshape(-1) for a in colours + overlays])]


def test_result_does_not_depend_on_scratch(ctx):
    """the job records, the packed palette and the blend table travel in the staged table, the call's only scratch"""
    sweep.sweep(ctx, "render-labels")


# ---- invalid arguments: WSC_ERR_INVALID that names the argument, and no launch --------------------------------------------------------
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


INVALID = [
    ("labels_dev", dict(labels=None)), ("src_hw_host", dict(src=None)), ("out_hw_host", dict(out=None)),
    ("labels_off_host", dict(lab_off=None)), ("out_off_host", dict(out_off=None)), ("palette_host", dict(palette=None)),
    ("other_rgb_host", dict(other=None)), ("colour_dev", dict(colour=None)), ("img_dev", dict(img=None)),
    ("blend_host", dict(blend=None)), ("label_type", dict(label_type=2)), ("B=0", dict(B=0)), ("B=65536", dict(B=65536)),
    ("n_colours=0", dict(n_colours=0)), ("n_colours=64", dict(n_colours=64)),
    ("src_hw", dict(src=_i32([[4, 0], [2, 2]]))), ("src_hw", dict(src=_i32([[4, 4], [65536, 32768]]))),
    ("out_hw", dict(out=_i32([[0, 3], [2, 2]]))), ("out_hw", dict(out=_i32([[3, 3], [46341, 46341]]))),
    ("mid_hw", dict(mid=_i32([[0, 5], [0, 0]]))), ("mid_hw", dict(mid=_i32([[-1, -1], [0, 0]]))),
    ("mid_hw", dict(mid=_i32([[0, 0], [65536, 32768]]))),
    ("labels_off", dict(lab_off=np.array([0, -1], np.int64))), ("out_off", dict(out_off=np.array([-3, 27], np.int64))),
]


@pytest.mark.parametrize("names,change", INVALID, ids=["%s-%d" % (n, i) for i, (n, _) in enumerate(INVALID)])
def test_invalid_argument_is_refused_before_any_launch(ctx, names, change):
    a = dict(labels=ctx.to_device(np.zeros(8, np.int32)), label_type=1, B=2, src=_i32([[2, 2], [2, 2]]), mid=None, out=_i32([[3, 3], [2, 2]]),
             lab_off=np.array([0, 4], np.int64), out_off=np.array([0, 27], np.int64), palette=np.full((3, 3), 200, np.uint8), n_colours=3,
             other=np.zeros(3, np.uint8), img=ctx.to_device(np.zeros(39, np.uint8)), blend=np.zeros((4, 3, 256), np.uint8),
             colour=ctx.to_device(np.full(39, BAND, np.uint8)), overlay=ctx.to_device(np.full(39, BAND, np.uint8)))
    outputs = (a["colour"], a["overlay"])
    a.update(change)
    p = lambda v: None if v is None else ctypes.c_void_p(_lib._ptr(v))
    status = ctx._lib.wsc_render_labels(ctx.h, p(a["labels"]), a["label_type"], a["B"], p(a["src"]), p(a["mid"]), p(a["out"]), p(a["lab_off"]),
                                        p(a["out_off"]), p(a["palette"]), a["n_colours"], p(a["other"]), p(a["img"]), p(a["blend"]),
                                        p(a["colour"]), p(a["overlay"]))
    assert status == _lib.WSC_ERR_INVALID
    text = ctx._lib.wsc_last_error().decode()
    assert "wsc_render_labels" in text and names.split("=")[0] in text, text
    for buf in outputs:
        assert (ctx.to_host(buf, (39,), np.uint8) == BAND).all(), "an output was written"


def test_the_valid_form_of_the_invalid_argument_cases_runs(ctx):
    """the unchanged argument set of the test above is a legal call"""
    lab = np.array([0, 1, 2, 3, 1, 1, 0, 7], np.int32)
    colours, _ = render.render_labels(ctx, [lab[:4].reshape(2, 2), lab[4:].reshape(2, 2)], [(2, 2), (2, 2)], [(3, 3), (2, 2)],
                                      np.full((3, 3), 200, np.uint8))
    assert colours[0][:, :, 0].tolist() == [[200, 200, 200], [200, 200, 200], [200, 200, 0]]
    assert colours[1][:, :, 0].tolist() == [[200, 200], [200, 0]]


# ---- the stages that take should_saveimg --------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path))


def _files(d):
    return sorted(os.listdir(d)) if os.path.isdir(d) else []


def test_hsn_segment_writes_the_debug_images(tmp_path):
    """hsn.demo.segment at the sizes and with the synthetic models of tests/test_gpu_net.py::test_hsn_segment_driver (its `resized`
    case: originals of 375 x 500 and 300 x 290): exactly <name>.png and <name>_overlay.png per image, their decoded pixels equal to
    the oracle applied to the returned label maps, label maps bit-identical with and without the flag, no file without out_dir."""
    from oracle import cnn_ref
    from tests.test_gpu_net import _model
    from wsscam.hsn import demo as hsn_demo
    from wsscam.net import vgg16_cam

    C = 5
    sd_fg = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, True, seed=11)
    sd_bg = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, True, seed=12)
    models = {"fg": _model(vgg16_cam.CAM, sd_fg, C, _lib.PREC_F16X3), "bg": _model(vgg16_cam.CAM, sd_bg, C, _lib.PREC_F16X3)}
    alphas = {"fg": cnn_ref.grad_cam_weights(sd_fg, "vgg16", cnn_ref.VGG16_CFG, 33, C),
              "bg": cnn_ref.grad_cam_weights(sd_bg, "vgg16", cnn_ref.VGG16_CFG, 33, C)}
    rng = np.random.default_rng(13)
    images = [cnn_ref.synth_image(rng, 375, 500), cnn_ref.synth_image(rng, 300, 290)]
    names = ["2007_000033", "2007_000042"]
    kw = dict(models=models, alphas=alphas, is_verbose=False)
    cwd = sorted(os.listdir("."))
    plain = hsn_demo.segment("VOC2012", "VGG16", 2, images=[im.copy() for im in images], should_saveimg=False, **kw)
    silent = hsn_demo.segment("VOC2012", "VGG16", 2, images=[im.copy() for im in images], should_saveimg=True, **kw)
    assert sorted(os.listdir(".")) == cwd and _files(str(tmp_path)) == []  # no out_dir: nothing is written
    out = hsn_demo.segment("VOC2012", "VGG16", 2, images=[im.copy() for im in images], should_saveimg=True, out_dir=str(tmp_path),
                           names=names, **kw)
    for a, b, c in zip(plain, silent, out):
        assert a.dtype == c.dtype and np.array_equal(a, b) and np.array_equal(a, c)
    assert _files(str(tmp_path)) == sorted([n + e for n in names for e in (".png", "_overlay.png")])
    assert len({int(v) for m in out for v in np.unique(m)}) > 1  # (more than one colour is drawn)
    for name, lab, im in zip(names, out, images):
        colour, over = ref.render(np.uint8(lab), render.VOC_COLOURS, im.shape[:2], img=im, overlay_r=0.75)
        assert np.array_equal(_png(str(tmp_path / (name + ".png"))), colour)
        assert np.array_equal(_png(str(tmp_path / (name + "_overlay.png"))), over)


def test_hsn_deepglobe_debug_images_at_a_quarter(ctx, tmp_path):
    """03c_hsn/demo.py:223-232 on given label maps: S x S -> the original size -> dsize=(shape[0] // 4, shape[1] // 4), the image
    through cv2's 8-bit INTER_LINEAR (the oracle's loop statement of it), OVERLAY_R = 0.25; label 6 ('unknown') is no colour"""
    from oracle import hsn_ref
    from wsscam.hsn import demo as hsn_demo

    rng = np.random.default_rng(21)
    labs = [rng.integers(0, 7, (33, 33)).astype(np.int64) for _ in range(2)]
    images = [rng.integers(0, 256, (48, 48, 3)).astype(np.uint8), rng.integers(0, 256, (50, 37, 3)).astype(np.uint8)]
    hsn_demo.save_debug_images(ctx, "DeepGlobe", labs, images, ["a", "b"], str(tmp_path))
    assert _files(str(tmp_path)) == ["a.png", "a_overlay.png", "b.png", "b_overlay.png"]
    colours = render.colours_for("DeepGlobe")
    assert len(colours) == 6
    for name, lab, im in zip("ab", labs, images):
        q = (im.shape[1] // 4, im.shape[0] // 4)  # (height, width) of dsize=(shape[0] // 4, shape[1] // 4)
        small = hsn_ref.read_batch_u8([im], q)[0]
        colour, over = ref.render(lab, colours, q, mid_hw=im.shape[:2], img=small, overlay_r=0.25)
        assert np.array_equal(_png(str(tmp_path / (name + ".png"))), colour)
        assert np.array_equal(_png(str(tmp_path / (name + "_overlay.png"))), over)


def test_label_evaluator_writes_the_two_stage_images(ctx, tmp_path):
    """LabelEvaluator with out_size reduced to 40 x 40: 17 x 17 -> 40 x 40 -> the 52 x 52 original, from the prediction the counting
    pass leaves on the device; the confusion matrix is the one of a run without the images"""
    from wsscam.hsn import demo as hsn_demo

    rng = np.random.default_rng(22)
    colours = render.colours_for("ADP-func")
    labs = [rng.integers(0, 5, (17, 17)).astype(np.int64) for _ in range(3)]
    gts = [np.asarray(colours, np.uint8)[rng.integers(0, 5, (40, 40))] for _ in range(3)]
    images = [rng.integers(0, 256, (52, 52, 3)).astype(np.uint8) for _ in range(3)]
    names = ["p0", "p1", "p2"]
    ev, plain = hsn_demo.LabelEvaluator(ctx, colours, out_size=(40, 40)), hsn_demo.LabelEvaluator(ctx, colours, out_size=(40, 40))
    ev.update(labs, gts, saveimg_dir=str(tmp_path), images=images, names=names)
    plain.update(labs, gts)
    assert np.array_equal(ev.metrics()["confusion_matrix"], plain.metrics()["confusion_matrix"])
    assert _files(str(tmp_path)) == sorted([n + e for n in names for e in (".png", "_overlay.png")])
    for name, lab, im in zip(names, labs, images):
        colour, over = ref.render(lab, colours, (52, 52), mid_hw=(40, 40), img=im, overlay_r=0.75)
        assert np.array_equal(_png(str(tmp_path / (name + ".png"))), colour)
        assert np.array_equal(_png(str(tmp_path / (name + "_overlay.png"))), over)


def _synthetic_cues(rng, n_img, n_classes):
    """exclusive seeds: every seed pixel belongs to at most one class; about a third to none"""
    from wsscam.cues.demo import SEED_SIZE

    cues, labs = {}, []
    for i in range(n_img):
        lab = rng.integers(0, n_classes, (SEED_SIZE, SEED_SIZE))
        keep = rng.random((SEED_SIZE, SEED_SIZE)) < 0.67
        r, c = np.nonzero(keep)
        cues["%d_cues" % i] = np.stack([lab[r, c], r, c]).astype(np.int64)
        labs.append((lab, keep))
    return cues, labs


def test_eval_cues_writes_the_float_form(ctx, tmp_path):
    """02_cues/demo.py:467-477: the float rule -- VOC2012 at the ground truth's size with OVERLAY_R 0.75 (a pixel no class claims
    is the background, colour 0), and DeepGlobe 16 x 16 -> 4 x 4 with 0.25 (such a pixel takes `ignore_ind`: no colour)"""
    from oracle import hsn_ref
    from wsscam.cues import demo as cues_demo

    rng = np.random.default_rng(23)
    # VOC2012
    cues, labs = _synthetic_cues(rng, 2, 21)
    hw = [(37, 53), (20, 31)]
    gts = [rng.integers(0, 21, s).astype(np.uint8) for s in hw]
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in hw]
    voc_dir = tmp_path / "voc"
    cues_demo.eval_cues("VOC2012", "VGG16", 0.2, 2, should_saveimg=True, is_verbose=False, cues=cues, gts=gts, out_dir=str(tmp_path / "m"),
                        ctx=ctx, images=images, names=["x", "y"], img_out_dir=str(voc_dir))
    assert _files(str(voc_dir)) == ["x.png", "x_overlay.png", "y.png", "y_overlay.png"]
    for name, (lab, keep), s, im in zip("xy", labs, hw, images):
        colour, over = ref.render(np.where(keep, lab, 0), render.VOC_COLOURS, s, img=im, overlay_r=0.75, rule="float256")
        assert np.array_equal(_png(str(voc_dir / (name + ".png"))), colour)
        assert np.array_equal(_png(str(voc_dir / (name + "_overlay.png"))), over)
    # DeepGlobe
    colours = render.colours_for("DeepGlobe")
    cues, labs = _synthetic_cues(rng, 1, 6)
    gt = np.asarray(colours, np.uint8)[rng.integers(0, 6, (16, 16))]
    im = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    dg_dir = tmp_path / "dg"
    cues_demo.eval_cues("DeepGlobe", "VGG16", 0.2, 2, should_saveimg=True, is_verbose=False, cues=cues, gts=[gt], out_dir=str(tmp_path / "m"),
                        ctx=ctx, images=[im], names=["z"], img_out_dir=str(dg_dir))
    assert _files(str(dg_dir)) == ["z.png", "z_overlay.png"]
    lab, keep = labs[0]
    colour, over = ref.render(np.where(keep, lab, 6), colours, (4, 4), mid_hw=(16, 16), img=hsn_ref.read_batch_u8([im], (4, 4))[0],
                              overlay_r=0.25, rule="float256")
    assert colour.shape == (4, 4, 3)
    assert np.array_equal(_png(str(dg_dir / "z.png")), colour)
    assert np.array_equal(_png(str(dg_dir / "z_overlay.png")), over)
    # without a directory for them, in-memory images write nothing
    before = sorted(os.listdir("."))
    cues_demo.eval_cues("DeepGlobe", "VGG16", 0.2, 2, should_saveimg=True, is_verbose=False, cues=cues, gts=[gt], out_dir=str(tmp_path / "m"),
                        ctx=ctx, images=[im], names=["z"])
    assert sorted(os.listdir(".")) == before


@pytest.mark.parametrize("should_overlay", [True, False])
def test_seg_evaluator_writes_three_files_per_id(ctx, tmp_path, should_overlay):
    """SegEvaluator(saveimg_dir=...) at the two smallest maps of tests/test_gpu_seg_eval.py's evaluator case (image 1 larger than its
    ground truth: the image shown is cv2's 8-bit resize of it): <id>_img.png, <id>_output.png, <id>_pred.png against the oracle
    applied to the evaluator's own labels"""
    from tests import helpers
    from tests.test_gpu_seg_eval import EVAL_SIZES, VOC_TEST, _eval_case
    from wsscam import secdsrg
    from wsscam.voc12.dataloader import resize_bilinear_u8

    C = 6
    rng = np.random.default_rng(906)
    probs, images, gts = _eval_case(rng, C, None, EVAL_SIZES[:2], big_image=1)
    palette = rng.integers(0, 256, (C, 3)).astype(np.uint8)
    ids = ["2008_000009", b"2008_000016"]
    ev = secdsrg.SegEvaluator(C, VOC_TEST, ctx=ctx, saveimg_dir=str(tmp_path), should_overlay=should_overlay, palette=palette)
    plain = secdsrg.SegEvaluator(C, VOC_TEST, ctx=ctx)
    try:
        labels = ev.update(probs, images, gts, want_pred=True, ids=ids)
        same = plain.update(probs, images, gts, want_pred=True)
        assert all(np.array_equal(a, b) for a, b in zip(labels, same))
    finally:
        ev.close()
        plain.close()
    names = ["2008_000009", "2008_000016"]
    assert _files(str(tmp_path)) == sorted([n + e for n in names for e in ("_img.png", "_output.png", "_pred.png")])
    for name, lab, im, (_, hw) in zip(names, labels, images, EVAL_SIZES[:2]):
        shown = im if im.shape[:2] == hw else resize_bilinear_u8(im, hw)
        colour, over = ref.render(lab, palette, hw, other_rgb=(255, 255, 255), img=shown, overlay_r=0.75)
        assert np.array_equal(_png(str(tmp_path / (name + "_img.png"))), shown)
        assert np.array_equal(_png(str(tmp_path / (name + "_pred.png"))), colour)
        assert np.array_equal(_png(str(tmp_path / (name + "_output.png"))), over if should_overlay else colour)
    with pytest.raises(ValueError):
        secdsrg.SegEvaluator(C, VOC_TEST, ctx=ctx, saveimg_dir=str(tmp_path))  # no palette


def test_eval_cues_adp_writes_the_images_under_the_callers_names(tmp_path):
    """02_cues/demo.py:604-608 through eval_cues_adp(should_saveimg=True, names, img_out_dirs), the model and images of
    tests/test_gpu_net.py::test_eval_cues_adp_vs_reference_loop: per HTT type one pair of files per IMAGE name (three names for a
    batch size of two: the second batch is written too), np.uint8 rule, R = 0.75, 41 x 41 -> size x size, against the oracle on the
    returned cues"""
    from oracle import cnn_ref
    from tests.test_gpu_edge import _adp_like_image
    from tests.test_gpu_net import _model
    from wsscam.cues import demo as cues_demo
    from wsscam.net import vgg16_cam

    C, S = 31, 224
    sd = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, False, seed=33)
    model = _model(vgg16_cam.CAM, sd, C, _lib.PREC_F16X3)
    rng = np.random.default_rng(34)
    images = [_adp_like_image(rng, S, S) for _ in range(3)]
    alpha = cnn_ref.grad_cam_weights(sd, "vgg16", cnn_ref.VGG16_CFG, 33, C)
    gts = {h: [np.asarray(render.colours_for("ADP-" + h), np.uint8)[rng.integers(0, len(render.colours_for("ADP-" + h)), (S, S))] for _ in images]
           for h in ("morph", "func")}
    names = ["patch_a.png", "patch_b.png", "E.M.S.png"]
    dirs = {h: str(tmp_path / h) for h in ("morph", "func")}
    out, cues = cues_demo.eval_cues_adp("VGG16", "ADP_tuning_VGG16", 2, S, "tuning", True, False, model=model, alpha=alpha,
                                        thresholds=np.full((1, C), 0.5), images=images, gts=gts, out_dir=str(tmp_path / "m"), names=names,
                                        img_out_dirs=dirs)
    plain, _ = cues_demo.eval_cues_adp("VGG16", "ADP_tuning_VGG16", 2, S, "tuning", False, False, model=model, alpha=alpha,
                                       thresholds=np.full((1, C), 0.5), images=images, gts=gts, out_dir=str(tmp_path / "m"))
    for h in ("morph", "func"):
        assert out[h]["classes"][0] == "Background" and np.array_equal(out[h]["intersects"], plain[h]["intersects"])
        assert _files(dirs[h]) == sorted([n[:-4] + e for n in names for e in (".png", "_overlay.png")])
        colours = render.colours_for("ADP-" + h)
        drawn = 0
        for j, (name, im) in enumerate(zip(names, images)):
            lab = cues_demo.cue_label_map(cues[h]["%d_cues" % j], len(colours), empty_label=len(colours))
            drawn += int((lab < len(colours)).sum())
            colour, over = ref.render(lab, colours, (S, S), img=im, overlay_r=0.75)
            assert np.array_equal(_png(os.path.join(dirs[h], name[:-4] + ".png")), colour)
            assert np.array_equal(_png(os.path.join(dirs[h], name[:-4] + "_overlay.png")), over)
        assert drawn > 0  # some seeds exist


def test_eval_cues_reference_call_form_names_the_files_as_the_reference_does(ctx, tmp_path, monkeypatch):
    """eval_cues(dataset, model_type, thresh, batch_size, should_saveimg=True) with everything read from a settings tree (the cues
    from the pickle under ./eval/<sess_id>): the images land in ./out/<sess_id>/ as <name>.png and <name>_overlay.png, <name> the
    file name without '.jpg' -- the ground truth's own file names (<name>.png) are not what they are named by"""
    import pickle

    from oracle import hsn_ref
    from PIL import Image

    from wsscam import keras_store
    from wsscam.cues import demo as cues_demo

    db = tmp_path / "database"
    dg = db / "DGdevkit"
    for d in ("JPEGImages", "SegmentationClassAug", os.path.join("ImageSets", "Segmentation")):
        os.makedirs(dg / d)
    ini = tmp_path / "settings.ini"
    ini.write_text("[Download Directory]\ndata_dir = %s\n\n[Data Folders]\nmodel_cnn_dir = models_cnn\ncues_dir = cues\n" % db)
    rng = np.random.default_rng(41)
    colours = render.colours_for("DeepGlobe")
    files = ["tile_1.jpg", "tile_2.jpg"]
    header = "Patch Names," + ",".join(keras_store.DEEPGLOBE_CLASSES)
    rows = [f + "," + ",".join("1" for _ in keras_store.DEEPGLOBE_CLASSES) for f in files]
    (dg / "ImageSets" / "Segmentation" / "train75.csv").write_text(header + "\n" + rows[0] + "\n")
    (dg / "ImageSets" / "Segmentation" / "test.csv").write_text(header + "\n" + "\n".join(rows) + "\n")
    gts = []
    for f in files:
        Image.fromarray(rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)).save(str(dg / "JPEGImages" / f), quality=95)
        gts.append(np.asarray(colours, np.uint8)[rng.integers(0, 6, (16, 16))])
        Image.fromarray(gts[-1]).save(str(dg / "SegmentationClassAug" / f.replace(".jpg", ".png")))
    cues, labs = _synthetic_cues(rng, 2, 6)
    monkeypatch.chdir(tmp_path)
    os.makedirs(os.path.join("eval", "DeepGlobe_VGG16"))
    with open(os.path.join("eval", "DeepGlobe_VGG16", "localization_cues_val.pickle"), "wb") as f:
        pickle.dump(cues, f)
    cues_demo.eval_cues("DeepGlobe", "VGG16", 0.2, 2, should_saveimg=True, is_verbose=False, ctx=ctx, settings=str(ini))
    out_dir = os.path.join("out", "DeepGlobe_VGG16")
    assert _files(out_dir) == ["tile_1.png", "tile_1_overlay.png", "tile_2.png", "tile_2_overlay.png"]
    for f, (lab, keep) in zip(files, labs):
        im = np.asarray(Image.open(str(dg / "JPEGImages" / f)).convert("RGB"))
        colour, over = ref.render(np.where(keep, lab, 6), colours, (4, 4), mid_hw=(16, 16), img=hsn_ref.read_batch_u8([im], (4, 4))[0],
                                  overlay_r=0.25, rule="float256")
        assert np.array_equal(_png(os.path.join(out_dir, f[:-4] + ".png")), colour)
        assert np.array_equal(_png(os.path.join(out_dir, f[:-4] + "_overlay.png")), over)


def test_segment_adp_without_names_numbers_the_files_and_refuses_a_wrong_count():
    from wsscam.hsn import demo as hsn_demo

    with pytest.raises(ValueError, match="2 names for 3 images"):
        hsn_demo.segment_adp(None, None, None, [None] * 3, None, 224, 2, should_saveimg=True, out_dirs={"morph": "a", "func": "b"},
                             names=["x", "y"])


from tests.test_gpu_seg_train_loop import data  # noqa: E402,F401  (the module's fixture: six PNGs, ground truths, cue lists)


def test_train_loop_validation_writes_the_saveimg_files(ctx, data, tmp_path):
    """--saveimg of Model.train (model.py:513-524, :721-728) on the thin DSRG net of tests/test_gpu_seg_train_loop.py: at every report
    <out_dir>/train/<i>/ holds <id>_img.png = np.uint8(img[j] + img_mean) of the network's own input, and <id>_output.png =
    <id>_pred.png = label2rgb of the arg-max (should_overlay is False in that call); VOC2012 keeps image 0 of every batch"""
    from tests import test_gpu_seg_train_loop as tl
    from wsscam import secdsrg

    ids, cues, load_image, load_gt = data
    val_ids = ids[1:4]  # two batches: 2 + 1
    palette = np.random.default_rng(51).integers(0, 256, (tl.C, 3)).astype(np.uint8)
    with secdsrg.SegTrainLoop("DSRG", tl._weights("DSRG"), tl.C, ids, load_image, cues, val_sets={"val": (val_ids, load_image, load_gt)},
                              should_saveimg=True, out_dir=str(tmp_path), dataset="VOC2012", palette=palette,
                              **tl._kwargs(ctx, 4, 0.0, max_epochs=1)) as loop:  # (accum_num beyond the run: the weights stay)
        reports = loop.run()
        images, gts = [load_image(i) for i in val_ids], [load_gt(i) for i in val_ids]
        x, gt_dev = loop.batcher.val_batch(images, gts)
        with x, gt_dev:
            with loop.trainer.net.rescale_output_dev(x, tl.MEAN, tl.CRF_CFG, seed_size=tl.SEED_SIZE) as out:
                pred = np.argmax(out.to_host(), axis=-1)
            shown = [np.uint8(im + np.asarray(tl.MEAN, np.float64).reshape(1, 1, 3)) for im in x.to_host()]
    plain = None
    with secdsrg.SegTrainLoop("DSRG", tl._weights("DSRG"), tl.C, ids, load_image, cues, val_sets={"val": (val_ids, load_image, load_gt)},
                              **tl._kwargs(ctx, 4, 0.0, max_epochs=1)) as loop:
        plain = loop.run()
    assert [r["miou"] for r in reports] == [r["miou"] for r in plain]
    assert _files(str(tmp_path / "train")) == [str(r["iteration"]) for r in reports] == ["0", "2"]
    kept = [0, 2]  # image 0 of the batches (img1, img2) and (img3)
    for i in ("0", "2"):
        d = tmp_path / "train" / i
        assert _files(str(d)) == sorted([val_ids[k] + e for k in kept for e in ("_img.png", "_output.png", "_pred.png")])
        for k in kept:
            colour, _ = ref.render(pred[k], palette, pred[k].shape, other_rgb=(255, 255, 255))
            assert np.array_equal(_png(str(d / (val_ids[k] + "_img.png"))), shown[k])
            assert np.array_equal(_png(str(d / (val_ids[k] + "_pred.png"))), colour)
            assert np.array_equal(_png(str(d / (val_ids[k] + "_output.png"))), colour)
    with pytest.raises(ValueError, match="palette"):
        secdsrg.SegTrainLoop("DSRG", None, tl.C, ids, load_image, cues, should_saveimg=True, out_dir=str(tmp_path), **tl._kwargs(ctx, 1, 0.0))
