"""CPU: the seed oracle of tests/cue_seeds_ref.py against the host functions of wsscam.cues.utilities (the mirrors of
02_cues/utilities.py:183-278 and 02_cues/adp_cues.py:304-339), its building blocks against numpy / scipy, the hand-made
cases against their constructed answers, and the host half of the device path (cues_from_label_maps, the exports)."""
import numpy as np
import pytest
import scipy.ndimage

from tests import cue_seeds_ref as ref
from wsscam.cues import utilities as cues

THRESH = 0.2  # the reference's default seed threshold (02_cues/demo.py)


@pytest.fixture(scope="module")
def sweep():
    """[(name, fg, bg or None)], generated once."""
    return ref.sweep_cases()


def _host_labels(fn, *args):
    out = {}
    B, H, W = args[0].shape[0], args[0].shape[2], args[0].shape[3]
    fn(out, *args[:-1], [np.zeros(0, int)] * B, list(range(B)), args[-1])
    return ref.labels_from_cues(out, range(B), H, W)


def test_oracle_equals_host_functions(sweep):
    """On every pixel that is not ambiguous -- no other exclusion -- and the ambiguous ones are few (a condition on the inputs)."""
    ambiguous = total = 0
    for name, fg, bg in sweep:
        f64 = fg.astype(np.float64)
        runs = [(_host_labels(cues.get_fg_cues, f64, THRESH), ref.seeds(fg, None, THRESH)),
                (_host_labels(cues.update_cues_adp, f64, THRESH), ref.seeds(fg, None, THRESH, per_image_max=True))]
        if bg is not None:
            runs.append((_host_labels(cues.get_fgbg_cues, f64, bg.astype(np.float64), THRESH), ref.seeds(fg, bg, THRESH)))
        for host, (lab, area, amb) in runs:
            assert np.array_equal(host[~amb], lab[~amb]), name
            ambiguous += int(amb.sum())
            total += amb.size
    assert ambiguous <= 0.05 * total, (ambiguous, total)


def test_sequential_sum_is_numpy_sum():
    """np.sum(axis=0) of a float64 stack adds the channels one after the other: 29 channels over 11 decades."""
    rng = np.random.default_rng(5)
    stack = rng.random((29, 41, 41)) * np.logspace(-6, 5, 29)[rng.permutation(29)][:, None, None]
    assert np.array_equal(np.sum(stack, axis=0), ref.sequential_sum(stack))
    s32 = stack.astype(np.float32)
    assert np.array_equal(np.sum(s32.astype(np.float64), axis=0), ref.sequential_sum(s32))
    assert not np.array_equal(ref.sequential_sum(s32), ref.sequential_sum(s32[::-1]))  # the order matters on this input


def test_median_and_rank_are_scipy_and_sort(sweep):
    for name, fg, bg in sweep:
        if bg is None:
            continue
        for x in bg:
            s = ref.sequential_sum(x)
            med = ref.median3x3(s)
            assert np.array_equal(med, scipy.ndimage.median_filter(s, 3)), name
            k = int(0.1 * s.shape[0] * s.shape[1])
            assert np.array_equal(ref.background_mask(x), med < np.sort(med.ravel())[k]), name


def test_sweep_is_not_vacuous(sweep):
    bg_seeds = multi = 0
    equal_area_overlap = False
    for name, fg, bg in sweep:
        m = ref.masks(fg, bg, THRESH)
        lab, area, amb = ref.resolve(m)
        if bg is not None:
            bg_seeds += int((lab == 1).sum())
        multi += int((m.sum(axis=1) >= 2).sum())
        equal_area_overlap |= bool(amb.any())  # two covering masks of one pixel, both non-empty, with one area
    assert bg_seeds >= 100 and multi >= 1000 and equal_area_overlap, (bg_seeds, multi, equal_area_overlap)


@pytest.mark.parametrize("case", ref.handmade_cases(), ids=lambda c: c[0])
def test_handmade_answers(case):
    """The constructed answers; the properties that make a case what it is -- a float32 product misjudging a threshold
    neighbour, another summation order ranking another pixel -- are asserted where cue_seeds_ref builds the inputs."""
    name, fg, bg, kw, expect = case
    lab, area, amb = ref.seeds(fg, bg, **kw)
    assert area.shape == (fg.shape[0], fg.shape[1] + (bg is not None))
    if expect is not None:
        assert np.array_equal(lab, expect), name


def test_reflect_border_case_tells_borders_apart():
    """scipy's 'reflect' repeats the edge sample.  The case's answer differs under a constant, a 'mirror' and a 'wrap' border;
    with a 3 x 3 window 'nearest' repeats the same one sample, so no input can tell it from 'reflect'."""
    name, fg, bg, kw, _ = [c for c in ref.handmade_cases() if c[0] == "reflect-border"][0]
    s = ref.sequential_sum(bg[0])
    k = int(0.1 * s.size)
    want = ref.background_mask(bg[0])
    assert want.any() and not want.all()
    for mode, cval in (("constant", 0.0), ("constant", 1.0), ("mirror", 0.0), ("wrap", 0.0)):
        med = scipy.ndimage.median_filter(s, 3, mode=mode, cval=cval)
        assert not np.array_equal(med < np.sort(med.ravel())[k], want), (mode, cval)
    assert np.array_equal(scipy.ndimage.median_filter(s, 3, mode="nearest"), scipy.ndimage.median_filter(s, 3, mode="reflect"))


def test_exports(built):
    """wsc_cue_maps / wsc_cue_seeds are declared in the header, exported by the library and bound in _lib."""
    from wsscam import _lib

    declared = _lib.check_exports()
    assert "wsc_cue_seeds" in declared and "wsc_cue_maps" in declared


def test_cues_from_label_maps(sweep):
    """The '%d_cues' arrays of _resolve_and_store, exactly (dtype, shape, order), from the oracle's label maps -- on the
    tie-free images, where the two agree on every pixel -- and (3, 0) for an empty label map."""
    checked = 0
    for name, fg, bg in sweep:
        lab, area, amb = ref.seeds(fg, bg, THRESH)
        B = len(fg)
        class_inds = [np.arange(b + 1) for b in range(B)]
        host = {}
        if bg is None:
            cues.get_fg_cues(host, fg.astype(np.float64), class_inds, list(range(B)), THRESH)
        else:
            cues.get_fgbg_cues(host, fg.astype(np.float64), bg.astype(np.float64), class_inds, list(range(B)), THRESH)
        mine = cues.cues_from_label_maps({}, lab, class_inds, list(range(B)))
        assert sorted(mine) == sorted(host)
        for b in range(B):
            if amb[b].any():
                continue
            a, h = mine["%d_cues" % b], host["%d_cues" % b]
            assert a.dtype == h.dtype == np.int64 and a.shape == h.shape and np.array_equal(a, h), (name, b)
            assert mine["%d_labels" % b] is class_inds[b]
            checked += a.shape[1] > 0
    assert checked >= 10
    empty = cues.cues_from_label_maps({}, np.zeros((1, 5, 4), np.uint8), [np.zeros(0, int)], [7])
    want = np.array(np.where(np.zeros((3, 5, 4), np.int64)))
    assert empty["7_cues"].dtype == want.dtype == np.int64 and empty["7_cues"].shape == want.shape == (3, 0)
