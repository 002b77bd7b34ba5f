"""Host: the SEC / DSRG batch inputs' rules (tests/seg_batch_ref.py) as facts, and the package's host twins against them
(wsscam.secdsrg.SegBatcher.train_batch_host / val_batch_host, tf_nearest_index, shuffled_ids).  Every check is an equality."""
import itertools

import numpy as np
import pytest

from tests import seg_batch_ref as sref
from wsscam import secdsrg

MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
COLOURS = [(255, 255, 255), (3, 155, 229), (0, 0, 128), (0, 128, 0), (173, 20, 87)]


# ---- the nearest index ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(375, 321), (500, 321), (321, 321), (41, 321), (1, 33)])
def test_nearest_index_is_the_integer_rule_on_ordinary_sizes(n_in, n_out):
    assert np.array_equal(sref.nearest_index(n_in, n_out), sref.nearest_index_exact(n_in, n_out))


@pytest.mark.parametrize("n_in,n_out,dst", [(39, 33, 11), (77, 33, 27), (6, 321, 107)])
def test_nearest_index_is_float32(n_in, n_out, dst):
    got, exact = sref.nearest_index(n_in, n_out), sref.nearest_index_exact(n_in, n_out)
    assert got[dst] == exact[dst] - 1  # the float32 product falls just below the whole number
    if (n_in, n_out) == (39, 33):
        assert got[11] == 12 and exact[11] == 13
    assert np.array_equal(secdsrg.tf_nearest_index(n_in, n_out), got)


@pytest.mark.parametrize("n_in,n_out", [(39, 33), (77, 33), (6, 321), (375, 321), (1, 1), (50, 7)])
def test_package_nearest_index(n_in, n_out):
    assert np.array_equal(secdsrg.tf_nearest_index(n_in, n_out), sref.nearest_index(n_in, n_out))


# ---- cues and labels -------------------------------------------------------------------------------------------------------------------
def test_dense_cues_by_hand():
    # (class, row, col): class 1 at (0, 2), class 0 at (1, 1), class 1 at (2, 0), and the first entry once more
    triples = np.array([[1, 0, 1, 1], [0, 1, 2, 0], [2, 1, 0, 2]])
    want = np.zeros((1, 3, 3, 2), np.float32)
    want[0, 0, 2, 1] = want[0, 1, 1, 0] = want[0, 2, 0, 1] = 1.0
    assert np.array_equal(sref.dense_cues([triples], 3, 2), want)
    assert want.sum() == 3


def test_labels_with_an_empty_list():
    got = sref.labels([[], [2, 2, 4]], 5)
    assert np.array_equal(got, np.array([[1, 0, 0, 0, 0], [1, 0, 1, 0, 1]], np.float32))


# ---- the class tests -------------------------------------------------------------------------------------------------------------------
def test_class_tests():
    px = np.array([[(3, 155, 229), (3, 155, 228)], [(173, 20, 87), (255, 255, 255)]], np.uint8)
    assert np.array_equal(sref.class_index(px, 5, COLOURS), np.array([[1, 5], [4, 0]], np.uint8))  # an unlisted colour: n_class
    vals = np.array([[0, 4, 5, 255]], np.uint8)[:, :, None]
    assert np.array_equal(sref.class_index(vals, 5), np.array([[0, 4, 5, 5]], np.uint8))  # 255 (and 5): n_class


# ---- the package's host twins -------------------------------------------------------------------------------------------------------------
def _cue_case(s, C, seed=0):
    rng = np.random.default_rng(seed)
    full = np.array([(c, r, q) for r in range(s) for q in range(s) for c in range(C)]).T
    corners = np.array([[0, C - 1, 1 % C, C - 1, 0, C - 1], [0, 0, s - 1, s - 1, 0, s - 1], [0, s - 1, 0, s - 1, 0, s - 1]])
    rand = np.stack([rng.integers(0, C, 40), rng.integers(0, s, 40), rng.integers(0, s, 40)])
    data = {"a_cues": np.zeros((3, 0), np.int64), "a_labels": np.zeros((0,), np.int64), "b_cues": corners, "b_labels": np.array([C - 1]),
            "c_cues": full, "c_labels": np.arange(C), "d_cues": rand, "d_labels": np.array([1 % C, 1 % C])}
    return ["a", "b", "c", "d"], data


@pytest.mark.parametrize("s,C", [(5, 3), (9, 21)])
def test_train_batch_host(s, C):
    ids, data = _cue_case(s, C)
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((7, 5), (33, 41), (50, 23), (33, 33))]
    x, cues, labels = secdsrg.SegBatcher(C, MEAN, size=(33, 33), seed_size=s).train_batch_host(ids, images, data)
    assert np.array_equal(cues, sref.dense_cues([data[i + "_cues"] for i in ids], s, C)) and cues.dtype == np.float32
    assert np.array_equal(labels, sref.labels([data[i + "_labels"] for i in ids], C)) and labels.dtype == np.float32
    assert cues[0].sum() == 0 and cues[2].min() == 1.0 and labels[0].tolist() == [1.0] + [0.0] * (C - 1)
    assert x.shape == (4, 33, 33, 3) and x.dtype == np.float32
    assert np.array_equal(x[3], images[3][:, :, ::-1].astype(np.float32) - MEAN.reshape(1, 1, 3))  # equal sizes pass through
    bad = dict(data, b_cues=np.array([[0], [s], [0]]))
    with pytest.raises(ValueError, match="sample 1"):
        secdsrg.SegBatcher(C, MEAN, size=(33, 33), seed_size=s).train_batch_host(ids, images, bad)


def test_val_batch_host():
    rng = np.random.default_rng(2)
    col = np.array(COLOURS + [(1, 2, 3)], np.uint8)
    gt3 = col[rng.integers(0, 6, (39, 77))]
    gt1 = np.array([0, 1, 2, 3, 4, 255], np.uint8)[rng.integers(0, 6, (6, 39))]
    images = [rng.integers(0, 256, (5, 4, 3), dtype=np.uint8)] * 2
    for size in ((33, 33), (321, 33)):
        _, got = secdsrg.SegBatcher(5, MEAN, size=size, colours=COLOURS).val_batch_host(images, [gt3, gt3[:1, :1]])
        assert got.dtype == np.uint8 and np.array_equal(got[0], sref.gt_index(gt3, 5, size, COLOURS)) and (got[0] == 5).any()
        assert (got[1] == got[1][0, 0]).all()
        _, got = secdsrg.SegBatcher(5, MEAN, size=size).val_batch_host(images, [gt1, gt1[:, :, None]])
        assert np.array_equal(got[0], sref.gt_index(gt1, 5, size)) and np.array_equal(got[0], got[1]) and (got[0] == 5).any()


# ---- the shuffle order ------------------------------------------------------------------------------------------------------------------
def _take(n, seed, m, skip=0):
    return list(itertools.islice(secdsrg.shuffled_ids(n, seed, skip=skip), m))


@pytest.mark.parametrize("n", [1, 6, 17])
def test_shuffled_ids(n):
    m = 5 * n + 7
    got = _take(n, 3, m)
    rng = np.random.default_rng(3)
    assert got == sref.shuffle_order(n, [int(rng.integers(0, n)) for _ in range(m)])
    assert got == _take(n, 3, m) and (n == 1 or got != _take(n, 4, m))  # deterministic per seed
    for k in (0, 1, n, 2 * n + 3):
        assert _take(n, 3, m - k, skip=k) == got[k:]
    assert all(0 <= v < n for v in got)
    assert max(np.bincount(got, minlength=n)) <= m // n + 2


def test_latest_checkpoint(tmp_path):
    assert secdsrg.latest_checkpoint(str(tmp_path)) == (None, 0)
    for name in ("epoch-3.npy", "epoch-12.npy", "epoch-x.npy", "final-0.npy", "epoch-40.txt"):
        (tmp_path / name).write_bytes(b"")
    assert secdsrg.latest_checkpoint(str(tmp_path)) == (str(tmp_path / "epoch-12.npy"), 12)
