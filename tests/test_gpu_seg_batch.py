"""GPU: the SEC / DSRG batch inputs on the device (csrc/seg_batch.hip: wsc_seg_train_batch, wsc_seg_gt_index_tf;
secdsrg.SegBatcher; SegEvaluator(crf=False) on a device ground truth).

  train batch   x BIT-equal to SegNet.preprocess_dev of the same images, cues and labels equal to tests/seg_batch_ref.py, at three
                (seed size, classes) cases, with the cue buffer on and off the 16-byte grid; a batch with no entry at all
  gt index      every pixel equal to the restatement at sizes where the float32 nearest index differs from the integer rule
  errors        WSC_ERR_INVALID before any launch: the outputs keep their canaries
  evaluator     the confusion matrix of a device gt_index equals the one of the same ground truth given on the host
Every device output lies between guard bands of a canary value that must survive.  All comparisons are exact."""
import numpy as np
import pytest

from tests import deeplab_ref as ref
from tests import seg_batch_ref as sref
from wsscam import _lib, secdsrg
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
COLOURS = [(255, 255, 255), (3, 155, 229), (0, 0, 128), (0, 128, 0), (173, 20, 87)]
CANARY = np.float32(-777.25)
CANARY_U8 = np.uint8(0xA5)
GUARD = 256  # canary elements around every device output
SIZE = (33, 33)
IMAGE_HW = ((7, 5), (33, 41), (50, 23))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _images(seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in IMAGE_HW]


def _pack(ctx, arrays):
    flat = [np.ascontiguousarray(a).reshape(-1) for a in arrays]
    return DeviceMaps.from_host(ctx, np.concatenate(flat)), np.concatenate(([0], np.cumsum([f.size for f in flat])))[:-1]


def _guarded(ctx, n, lead, canary=CANARY):
    return DeviceMaps.from_host(ctx, np.full((lead + n + GUARD,), canary, np.asarray(canary).dtype))


def _body(buf, n, lead, what, canary=CANARY):
    flat = buf.to_host()
    assert (flat[:lead] == canary).all() and (flat[lead + n:] == canary).all(), what + ": a store outside the buffer"
    return flat[lead:lead + n].copy()


def _cue_lists(s, C):
    """one empty list, one with duplicates and the four corners, one with every (row, col, class) of the plane"""
    corners = np.array([[0, C - 1, 1 % C, C - 1, 0, C - 1, C - 1], [0, 0, s - 1, s - 1, 0, s - 1, s - 1], [0, s - 1, 0, s - 1, 0, s - 1, s - 1]])
    full = np.array([(c, r, q) for r in range(s) for q in range(s) for c in range(C)]).T
    return [np.zeros((3, 0), np.int64), corners, full], [[], [C - 1, C - 1], list(range(C))]


def _train_batch(ctx, images, tables, s, C, lead):
    """wsc_seg_train_batch on guarded outputs, the cue buffer `lead` floats off its allocation -> (x, cues, labels)"""
    B, (H, W) = len(images), SIZE
    n = (B * H * W * 3, B * s * s * C, B * C)
    packed, offsets = _pack(ctx, images)
    with packed, _guarded(ctx, n[0], GUARD) as xd, _guarded(ctx, n[1], lead) as cd, _guarded(ctx, n[2], GUARD) as ld:
        _lib.seg_train_batch(ctx, packed.ptr, [im.shape[:2] for im in images], offsets, *tables, MEAN, SIZE, s, C, xd.ptr + 4 * GUARD,
                             cd.ptr + 4 * lead, ld.ptr + 4 * GUARD)
        return (_body(xd, n[0], GUARD, "x").reshape(B, H, W, 3), _body(cd, n[1], lead, "cues").reshape(B, s, s, C),
                _body(ld, n[2], GUARD, "labels").reshape(B, C))


@pytest.fixture(scope="module")
def x_want(ctx):
    """SegNet.preprocess_dev of the test images: computed once, read only"""
    net = secdsrg.SegNet("SEC", ref.random_weights("SEC", 5, 64, 128, seed=1), 5, ctx=ctx)
    try:
        with net.preprocess_dev(_images(), MEAN, SIZE) as x:
            out = x.to_host()
    finally:
        net.close()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("s,C", [(5, 3), (9, 21), (41, 32)])
def test_train_batch(ctx, x_want, s, C):
    images = _images()
    cue_lists, label_lists = _cue_lists(s, C)
    want_c, want_l = sref.dense_cues(cue_lists, s, C), sref.labels(label_lists, C)
    tables = _lib.seg_cue_tables(cue_lists, label_lists)
    for lead in (GUARD, GUARD + 1, GUARD + 3):  # the plane's address on the 16-byte grid and off it
        x, cues, labels = _train_batch(ctx, images, tables, s, C, lead)
        assert np.array_equal(_bits(x), _bits(x_want)), int((_bits(x) != _bits(x_want)).sum())
        assert np.array_equal(_bits(cues), _bits(want_c)), (lead, int((cues != want_c).sum()))
        assert np.array_equal(_bits(labels), _bits(want_l))
    assert want_c[0].sum() == 0 and want_c[1].sum() == 4 and want_c[2].min() == 1.0
    # no entry in the whole batch
    empty = _lib.seg_cue_tables([np.zeros((3, 0), np.int64)] * 3, [[]] * 3)
    assert empty[1].tolist() == [0, 0, 0, 0]
    x, cues, labels = _train_batch(ctx, images, empty, s, C, GUARD + 2)
    assert np.array_equal(_bits(x), _bits(x_want)) and not cues.any() and np.array_equal(labels, sref.labels([[]] * 3, C))


def test_batcher_train_batch(ctx, x_want):
    s, C = 9, 5
    cue_lists, label_lists = _cue_lists(s, C)
    ids = ["a", "b", "c"]
    data = {}
    for i, c, l in zip(ids, cue_lists, label_lists):
        data[i + "_cues"], data[i + "_labels"] = c, np.asarray(l, np.int64)
    batcher = secdsrg.SegBatcher(C, MEAN, size=SIZE, seed_size=s, ctx=ctx)
    x, cues, labels = batcher.train_batch(ids, _images(), data)
    with x, cues, labels:
        assert (x.shape, cues.shape, labels.shape) == ((3, 33, 33, 3), (3, s, s, C), (3, C))
        hx, hc, hl = batcher.train_batch_host(ids, _images(), data)
        assert np.array_equal(_bits(x.to_host()), _bits(x_want))
        assert np.array_equal(cues.to_host(), sref.dense_cues(cue_lists, s, C)) and np.array_equal(cues.to_host(), hc)
        assert np.array_equal(labels.to_host(), sref.labels(label_lists, C)) and np.array_equal(labels.to_host(), hl)
        # (the twin's x: the same float32 products and sums, each rounded on its own, so the same bits)
        assert np.array_equal(_bits(hx), _bits(x_want)), int((_bits(hx) != _bits(x_want)).sum())


# ---- wsc_seg_gt_index_tf ---------------------------------------------------------------------------------------------------------------
def _gts():
    rng = np.random.default_rng(2)
    col = np.array(COLOURS + [(1, 2, 3)], np.uint8)
    gt3 = [col[rng.integers(0, 6, hw)] for hw in ((39, 77), (6, 39), (1, 1))]
    gt1 = [np.array([0, 1, 2, 3, 4, 255], np.uint8)[rng.integers(0, 6, hw)] for hw in ((6, 39), (39, 77), (1, 1))]
    return gt3, gt1


def _gt_index(ctx, gts, channels, colours, n_class, out_hw):
    B, n = len(gts), len(gts) * out_hw[0] * out_hw[1]
    packed, offsets = _pack(ctx, gts)
    with packed, _guarded(ctx, n, GUARD + 1, CANARY_U8) as out:
        _lib.seg_gt_index_tf(ctx, packed.ptr, [g.shape[:2] for g in gts], offsets, channels, colours, n_class, out_hw, out.ptr + GUARD + 1)
        return _body(out, n, GUARD + 1, "gt index", CANARY_U8).reshape(B, out_hw[0], out_hw[1])


@pytest.mark.parametrize("out_hw", [(33, 33), (321, 33)])
def test_gt_index(ctx, out_hw):
    gt3, gt1 = _gts()
    # (the sizes hold the float32-vs-integer cases: an index computed in integers or in double gives other pixels)
    assert (sref.nearest_index(39, 33) != sref.nearest_index_exact(39, 33)).any() and (sref.nearest_index(77, 33) != sref.nearest_index_exact(77, 33)).any()
    assert (sref.nearest_index(6, 321) != sref.nearest_index_exact(6, 321)).any()
    got = _gt_index(ctx, gt3, 3, COLOURS, 5, out_hw)
    for b, g in enumerate(gt3):
        want = sref.gt_index(g, 5, out_hw, COLOURS)
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
    assert (got[0] == 5).any()  # the unlisted colour
    got = _gt_index(ctx, gt1, 1, None, 5, out_hw)
    for b, g in enumerate(gt1):
        want = sref.gt_index(g, 5, out_hw)
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
    assert (got[0] == 5).any()  # 255
    got = _gt_index(ctx, gt3, 3, None, 5, out_hw)  # three channels, no table: channel 0
    for b, g in enumerate(gt3):
        assert np.array_equal(got[b], sref.gt_index(g, 5, out_hw))


def test_batcher_val_batch(ctx, x_want):
    gt3, gt1 = _gts()
    for colours, gts in ((COLOURS, gt3), (None, gt1)):
        batcher = secdsrg.SegBatcher(5, MEAN, size=SIZE, colours=colours, ctx=ctx)
        x, gt = batcher.val_batch(_images(), gts)
        with x, gt:
            assert gt.dtype == np.uint8 and gt.shape == (3, 33, 33)
            assert np.array_equal(_bits(x.to_host()), _bits(x_want))
            assert np.array_equal(gt.to_host(), np.stack([sref.gt_index(g, 5, SIZE, colours) for g in gts]))
            assert np.array_equal(gt.to_host(), batcher.val_batch_host(_images(), gts)[1])


# ---- errors before any launch ---------------------------------------------------------------------------------------------------------------
def test_train_batch_errors(ctx):
    s, C = 5, 3
    images = _images()
    sizes = [im.shape[:2] for im in images]
    cue_lists, label_lists = _cue_lists(s, C)
    good = _lib.seg_cue_tables(cue_lists, label_lists)

    def entry(row, value):  # sample 1's first entry with one field replaced
        c = cue_lists[1].copy()
        c[row, 0] = value
        return _lib.seg_cue_tables([cue_lists[0], c, cue_lists[2]], label_lists)

    def offsets(which, values):
        t = list(good)
        t[which] = np.array(values, np.int32)
        return tuple(t)

    n1 = cue_lists[1].shape[1]
    cases = [("class C", entry(0, C), {}, "sample 1"), ("class -1", entry(0, -1), {}, "sample 1"), ("row s", entry(1, s), {}, "sample 1"),
             ("row -1", entry(1, -1), {}, "sample 1"), ("col s", entry(2, s), {}, "sample 1"), ("col -1", entry(2, -1), {}, "sample 1"),
             ("label C", _lib.seg_cue_tables(cue_lists, [[], [C], [0]]), {}, "sample 1"),
             ("negative cue offset", offsets(1, [-1, 0, n1, n1 + s * s * C]), {}, "sample 0"),
             ("decreasing cue offset", offsets(1, [0, n1, n1 - 1, n1 + s * s * C]), {}, "sample 1"),
             ("negative label offset", offsets(3, [-1, 0, 2, 2 + C]), {}, "sample 0"),
             ("decreasing label offset", offsets(3, [0, 2, 1, 2 + C]), {}, "sample 1"),
             ("C = 0", good, {"C": 0}, "C=0"), ("C = 33", good, {"C": 33}, "C=33"), ("s * s > 8192", good, {"s": 91}, "s=91"),
             ("image offset", good, {"img_off": [0, -1, 0]}, "sample 1"), ("image size", good, {"sizes": [(7, 5), (0, 41), (50, 23)]}, "sample 1")]
    packed, img_off = _pack(ctx, images)
    n = (3 * 33 * 33 * 3, 3 * s * s * C, 3 * C)
    with packed, _guarded(ctx, n[0], GUARD) as xd, _guarded(ctx, n[1], GUARD) as cd, _guarded(ctx, n[2], GUARD) as ld:
        def call(tables, B_sizes=sizes, img_off=img_off, s=s, C=C):
            _lib.seg_train_batch(ctx, packed.ptr, B_sizes, img_off, *tables, MEAN, SIZE, s, C, xd.ptr + 4 * GUARD, cd.ptr + 4 * GUARD,
                                 ld.ptr + 4 * GUARD)

        for name, tables, kw, text in cases:
            with pytest.raises(_lib.WscError) as ei:
                call(tables, B_sizes=kw.get("sizes", sizes), img_off=np.array(kw.get("img_off", img_off)), s=kw.get("s", s), C=kw.get("C", C))
            assert ei.value.status == _lib.WSC_ERR_INVALID and text in str(ei.value), (name, str(ei.value))
        for B in (0, 65536):  # B outside 1 .. 65535
            with pytest.raises(_lib.WscError) as ei:
                z = np.zeros(B + 1, np.int32)
                call((good[0], z, good[2], z), B_sizes=np.ones((B, 2), np.int32), img_off=np.zeros(B, np.int64))
            assert ei.value.status == _lib.WSC_ERR_INVALID and "B=%d" % B in str(ei.value)
        for d, m in ((xd, n[0]), (cd, n[1]), (ld, n[2])):
            assert (d.to_host() == CANARY).all()  # nothing was launched
        call(good)  # ... and the same buffers take a valid call
        assert np.array_equal(_body(cd, n[1], GUARD, "cues").reshape(3, s, s, C), sref.dense_cues(cue_lists, s, C))


def test_gt_index_errors(ctx):
    gt3, gt1 = _gts()
    packed, off = _pack(ctx, gt3)
    sizes = [g.shape[:2] for g in gt3]
    n = 3 * 33 * 33
    with packed, _guarded(ctx, n, GUARD, CANARY_U8) as out:
        def call(sizes=sizes, off=off, channels=3, colours=COLOURS, n_class=5, out_hw=SIZE):
            _lib.seg_gt_index_tf(ctx, packed.ptr, sizes, off, channels, colours, n_class, out_hw, out.ptr + GUARD)

        cases = [dict(channels=1), dict(channels=2, colours=None), dict(n_class=0, colours=None), dict(n_class=33, colours=None),
                 dict(off=np.array([0, -3, 0])), dict(sizes=[(39, 77), (0, 39), (1, 1)]), dict(out_hw=(0, 33)),
                 dict(sizes=np.ones((0, 2), np.int32), off=np.zeros(0, np.int64)),
                 dict(sizes=np.ones((65536, 2), np.int32), off=np.zeros(65536, np.int64))]
        for kw in cases:
            with pytest.raises(_lib.WscError) as ei:
                call(**kw)
            assert ei.value.status == _lib.WSC_ERR_INVALID, kw
        assert (out.to_host() == CANARY_U8).all()  # nothing was launched
        call()
        assert np.array_equal(_body(out, n, GUARD, "gt index", CANARY_U8).reshape(3, 33, 33), np.stack([sref.gt_index(g, 5, SIZE, COLOURS) for g in gt3]))


# ---- SegEvaluator(crf=False) on a device ground truth ---------------------------------------------------------------------------------------
def test_evaluator_takes_a_device_gt_index(ctx):
    C, B, h, w = 5, 3, 33, 21
    rng = np.random.default_rng(9)
    probs = rng.random((B, h, w, C)).astype(np.float32)
    gt = rng.integers(0, C + 1, (B, h, w)).astype(np.uint8)  # C: a pixel of no class
    conf = []
    for on_device in (False, True):
        ev = secdsrg.SegEvaluator(C, None, ctx=ctx, crf=False)
        try:
            with DeviceMaps.from_host(ctx, probs) as pd, DeviceMaps.from_host(ctx, gt) as gd:
                pred = ev.update(pd, None, gd if on_device else list(gt), want_pred=True)
                assert np.array_equal(gd.to_host(), gt)
            assert np.array_equal(np.stack(pred), probs.argmax(-1).astype(np.uint8))
            conf.append(ctx.to_host(ev.conf_dev, (C + 1, C + 1), np.int64))
        finally:
            ev.close()
    want = np.zeros((C + 1, C + 1), np.int64)
    np.add.at(want, (gt.reshape(-1), probs.argmax(-1).reshape(-1)), 1)
    assert np.array_equal(conf[0], conf[1]) and np.array_equal(conf[1], want) and want[C].sum() > 0
    with DeviceMaps.from_host(ctx, probs) as pd, DeviceMaps.from_host(ctx, gt[:, :-1]) as gd:
        ev = secdsrg.SegEvaluator(C, None, ctx=ctx, crf=False)
        try:
            with pytest.raises(ValueError):
                ev.update(pd, None, gd)
        finally:
            ev.close()
