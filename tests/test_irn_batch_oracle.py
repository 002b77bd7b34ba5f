"""CPU: the numpy restatement of the IRNet training-sample transform (tests/irn_batch_ref.py) -- the oracle of
tests/test_gpu_irn_batch.py -- against PIL's Image.resize itself, against the host datasets' item(), and the draw order of the
crop box.  Everything here is an equality: no tolerance."""
import os
import random

import numpy as np
import pytest

from tests import irn_batch_ref as ref

FACTORS = (0.25, 0.5, 0.625, 0.75, 0.9, 1.0, 1.1, 1.25, 1.375, 1.5)


def _grid():
    """60 (image, factor) cases: sizes 5 .. 90, factors 0.25 and 0.5 .. 1.5, random and 0 / 255 images (both clamps fire)"""
    rng = np.random.default_rng(2024)
    cases = []
    for t in range(60):
        h, w = (int(v) for v in rng.integers(5, 91, 2))
        if t < 4:
            h, w = ((5, 90), (90, 5), (5, 5), (90, 90))[t]
        f = FACTORS[t % len(FACTORS)] if t % 3 else float(rng.uniform(0.5, 1.5))
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8) if t % 4 else (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        cases.append((img, f))
    return cases


def test_restatement_equals_pil_resize():
    Image = pytest.importorskip("PIL.Image")
    low = high = False
    for img, f in _grid():
        oh, ow = (max(v, 1) for v in ref.scaled_size(img.shape[:2], f))
        got = ref.pil_bicubic(img, (oh, ow))
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
        assert np.array_equal(got, want), (img.shape, f, int((got != want).sum()))
        lab = img[..., 0]
        got_l = ref.pil_nearest(lab, (oh, ow))
        want_l = np.asarray(Image.fromarray(lab).resize((ow, oh), Image.NEAREST))
        assert np.array_equal(got_l, want_l), (img.shape, f)
        got_1 = ref.pil_bicubic(lab, (oh, ow))  # mode L through the same 8-bit path
        assert np.array_equal(got_1, np.asarray(Image.fromarray(lab).resize((ow, oh), Image.BICUBIC)))
        if set(np.unique(img)) <= {0, 255} and f != 1.0:  # did a clamp fire? (the unclamped sum leaves 0 .. 255)
            tab = ref.resample_coeffs(img.shape[1], ow) if ow != img.shape[1] else []
            for xmin, n, coef in tab:
                acc = ((1 << 21) + np.tensordot(coef, img[:, xmin:xmin + n].astype(np.int64), axes=(0, 1))) >> 22
                low, high = low or bool((acc < 0).any()), high or bool((acc > 255).any())
    assert low and high, "the grid never reached a clamp"


def test_one_axis_kept_and_tiny():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for (h, w), (oh, ow) in (((37, 53), (37, 80)), ((37, 53), (19, 53)), ((2, 3), (5, 2)), ((37, 53), (19, 27)), ((37, 53), (56, 80))):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(ref.pil_bicubic(img, (oh, ow)), np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC)))
        assert np.array_equal(ref.pil_nearest(img[..., 1], (oh, ow)), np.asarray(Image.fromarray(img[..., 1]).resize((ow, oh), Image.NEAREST)))


def test_reduced_index_facts():
    assert ref.reduced_size(32) == 8 and ref.nearest_index(32, 8).tolist() == [2, 6, 10, 14, 18, 22, 26, 30]
    assert ref.reduced_size(34) == 8 and ref.nearest_index(34, 8).tolist()[-2:] == [27, 31]
    assert ref.reduced_size(30) == 8 and ref.nearest_index(30, 8).tolist()[:3] == [1, 5, 9]
    assert ref.reduced_size(512) == 128 and ref.reduced_size(64) == 16


def test_crop_box_draw_order(monkeypatch):
    """imutils.get_random_crop_box: two randrange draws, the width's first; the draw lands in img_* where the image is larger
    than the crop and in cont_* otherwise.  Expectations written by hand from a recorded call list."""
    from wsscam.misc import imutils

    calls = []

    def fake_randrange(n):
        calls.append(n)
        return n - 1  # the largest legal value

    monkeypatch.setattr(imutils.random, "randrange", fake_randrange)
    # larger on both axes: (h, w) = (40, 50), crop 32 -> w_space 18 first, then h_space 8; both draws go to img_*
    assert imutils.get_random_crop_box((40, 50), 32) == (0, 32, 0, 32, 8, 40, 18, 50)
    assert calls == [19, 9]
    calls.clear()
    # smaller on both axes: (20, 25) -> -w_space 7, -h_space 12; both draws go to cont_*
    assert imutils.get_random_crop_box((20, 25), 32) == (12, 32, 7, 32, 0, 20, 0, 25)
    assert calls == [8, 13]
    calls.clear()
    # wider but shorter: (20, 50) -> the width's draw to img_left, the height's to cont_top
    assert imutils.get_random_crop_box((20, 50), 32) == (12, 32, 0, 32, 0, 20, 18, 50)
    assert calls == [19, 13]
    calls.clear()
    # exactly the crop: one draw each from a range of one
    assert imutils.get_random_crop_box((32, 32), 32) == (0, 32, 0, 32, 0, 32, 0, 32)
    assert calls == [1, 1]
    monkeypatch.undo()
    # under a seeded `random` the box is the two randrange values, in that order
    random.seed(7)
    want_w, want_h = random.randrange(19), random.randrange(9)
    random.seed(7)
    assert imutils.get_random_crop_box((40, 50), 32) == (0, 32, 0, 32, want_h, want_h + 32, want_w, want_w + 32)


def test_draw_consumes_random_in_reference_order(tmp_path):
    """dataset.draw: random.random() (factor), getrandbits(1) (flip), then the box's two randrange"""
    ds, _ = synthetic_dataset(tmp_path, "voc12", rescale=(0.5, 1.5), crop_method="random", S=32)
    random.seed(11)
    p = ds.draw(1, (41, 57))
    random.seed(11)
    f = 0.5 + random.random() * 1.0
    sh, sw = int(np.round(41 * f)), int(np.round(57 * f))
    flip = random.getrandbits(1)
    from wsscam.misc import imutils

    b = imutils.get_random_crop_box((sh, sw), 32)
    assert p.tolist() == [sh, sw, flip, b[0], b[2], b[4], b[6], b[1] - b[0], b[3] - b[2]]


# ---- the host datasets' item() -----------------------------------------------------------------------------------------------------
SIZES = [(27, 41), (41, 57), (70, 30), (64, 64)]


def synthetic_dataset(root, kind, rescale=None, crop_method="random", S=32, outsize=None, norm_mode="int", sizes=SIZES):
    """4 synthetic PNGs (ADP / DeepGlobe: JPEG is lossy, so DeepGlobe's and VOC's '.jpg' files hold PNG data -- PIL decodes by
    content) with IR labels containing 0, 20, 21 and 255 -> (the affinity dataset, [(image, label)])"""
    Image = pytest.importorskip("PIL.Image")
    root = str(root)
    rng = np.random.default_rng(len(kind))
    names = {"voc12": ["2007_%06d" % (i + 1) for i in range(len(sizes))]}.get(kind, ["tile_%d" % i for i in range(len(sizes))])
    img_dir = os.path.join(root, {"voc12": "JPEGImages", "adp": "PNGImages", "deepglobe": "JPEGImages"}[kind])
    lab_dir = os.path.join(root, "ir_label")
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(lab_dir, exist_ok=True)
    data = []
    for name, (h, w) in zip(names, sizes):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        lab = rng.choice(np.array([0, 3, 20, 21, 255], np.uint8), (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w]
        Image.fromarray(img).save(os.path.join(img_dir, name + (".png" if kind == "adp" else ".jpg")), format="PNG")
        Image.fromarray(np.ascontiguousarray(lab)).save(os.path.join(lab_dir, name + ".png"))
        data.append((img, np.ascontiguousarray(lab)))
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as fh:
        fh.write("\n".join(names) + "\n")
    kw = dict(label_dir=lab_dir, crop_size=S, dev_root=root, rescale=rescale, norm_mode=norm_mode, hor_flip=True, crop_method=crop_method,
              outsize=outsize)
    if kind == "voc12":
        from wsscam.voc12.dataloader import VOC12AffinityDataset

        return VOC12AffinityDataset(lst, **kw), data
    if kind == "adp":
        from wsscam.adp.dataloader import ADPAffinityDataset

        return ADPAffinityDataset(lst, htt_type="morph", is_eval=False, **kw), data
    from wsscam.deepglobe.dataloader import DeepGlobeAffinityDataset

    return DeepGlobeAffinityDataset(lst, is_balanced=False, **kw), data


@pytest.mark.parametrize("kind,norm_mode,outsize", [("voc12", "int", None), ("voc12", "float", None), ("adp", "int", None),
                                                    ("deepglobe", "float", None), ("voc12", "int", (32, 32)), ("adp", "float", (32, 32))])
def test_restatement_equals_host_datasets(tmp_path, kind, norm_mode, outsize):
    S = 32
    ds, data = synthetic_dataset(tmp_path, kind, rescale=None if outsize else (0.5, 1.5), crop_method="random" if not outsize else "top_left",
                                 S=S, outsize=outsize, norm_mode=norm_mode)
    random.seed(3)
    seen_flip = set()
    for rep in range(3):
        for idx, (img, lab) in enumerate(data):
            dec = ds.decoded(idx)
            assert np.array_equal(dec[0], img) and np.array_equal(dec[1], lab)
            p = ds.draw(idx, img.shape[:2])
            seen_flip.add(int(p[2]))
            got = ds.item(idx, p)
            x, label, reduced = ref.transform(img, lab, p, S, ds.img_normal.mean, ds.img_normal.std, norm_mode == "float", 2 if outsize else 1)
            assert got["img"].dtype == np.float32 and got["label"].dtype == np.uint8 and got["reduced_label"].dtype == np.uint8
            assert np.array_equal(got["img"].view(np.uint32), x.view(np.uint32)), (kind, idx, p.tolist())
            assert np.array_equal(got["label"], label) and np.array_equal(got["reduced_label"], reduced), (kind, idx, p.tolist())
            assert got["reduced_label"].shape == (8, 8)
    assert seen_flip == {0, 1}
    item = ds[0]
    assert set(item) == {"name", "img", "label", "reduced_label"} and item["img"].shape == (3, S, S)


def test_rescale_with_outsize_is_an_error(tmp_path):
    with pytest.raises(ValueError):
        synthetic_dataset(tmp_path, "voc12", rescale=(0.5, 1.5), outsize=(32, 32))
