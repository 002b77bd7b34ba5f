"""CPU: the DSRG region-growing oracle (tests/dsrg_ref.py, vectorised numpy + scipy) against a per-pixel scan restatement of
03a_sec-dsrg/DSRG.py:7-62 with its own 8-neighbour union-find labeller -- in place and class after class, as the reference
runs -- and against hand-made cases whose answers are known by construction."""
import numpy as np
import pytest

from tests import dsrg_ref


def _components_8(mat):
    """Raster-scan two-pass labelling of a boolean map with a union-find; 0 = outside, components numbered from 1."""
    H, W = mat.shape
    parent = [0]

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    lab = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if not mat[y, x]:
                continue
            # the already visited neighbours: left, and the three of the row above
            near = [lab[yy][xx] for yy, xx in ((y, x - 1), (y - 1, x - 1), (y - 1, x), (y - 1, x + 1))
                    if 0 <= yy and 0 <= xx < W and lab[yy][xx]]
            if not near:
                parent.append(len(parent))
                lab[y][x] = len(parent) - 1
                continue
            roots = [find(n) for n in near]
            lab[y][x] = min(roots)
            for r in roots:
                parent[r] = lab[y][x]
    return [[find(v) if v else 0 for v in row] for row in lab]


def scan_seed_grow(tag, cue, prob, th_f=dsrg_ref.TH_F, th_b=dsrg_ref.TH_B):
    """The reference's procedure pixel by pixel: returns the grown cue (a copy; classes processed in order, in place)."""
    tag = np.asarray(tag, np.float32).reshape(-1)
    cue = np.array(cue, np.float32)
    H, W, C = cue.shape
    e = np.asarray(prob, np.float32) * tag
    cand = np.zeros((H, W), int)  # class + 1, 0 = none
    for y in range(H):
        for x in range(W):
            a = int(np.argmax(e[y, x]))
            fg = 1 if a >= 1 else 0
            fg_th = 1 if sum(1 for v in e[y, x, 1:] if v > np.float32(th_f)) > 0.5 else 0
            bg_th = 1 if e[y, x, 0] > np.float32(th_b) else 0
            cand[y, x] = (fg_th * fg + bg_th * (1 - fg)) * (a + 1)
    for c in range(C):
        if not tag[c] > 0.5:
            continue
        mat = cand == c + 1
        lab = _components_8(mat)
        hot = set()
        for y in range(H):
            for x in range(W):
                if mat[y, x] and cue[y, x, c] == 1:
                    hot.add(lab[y][x])
                elif mat[y, x] and cue[y, x].sum() == 1:
                    lab[y][x] = -1
        for y in range(H):
            for x in range(W):
                if lab[y][x] in hot:
                    cue[y, x, c] = 1
    return cue


@pytest.fixture(scope="module")
def sweep():
    return dsrg_ref.sweep_cases()


def test_components_labeller_is_8_connected():
    mat = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1]], bool)
    lab = np.array(_components_8(mat))
    assert lab[0, 0] == lab[1, 1] != 0                      # diagonal joins
    assert len({lab[0, 0], lab[0, 3], lab[2, 3], lab[3, 0]}) == 4  # four components in all
    assert lab[2, 3] == lab[3, 3] and (lab[~mat] == 0).all()


def test_oracle_equals_scan_on_generated_cases(sweep):
    grown = blocked = 0
    for name, tags, cues, probs in sweep:
        before = cues.copy()
        for b in range(len(cues)):
            out, g, k = dsrg_ref.seed_grow(tags[b], cues[b], probs[b])
            assert out.dtype == np.float32 and np.array_equal(out, scan_seed_grow(tags[b], cues[b], probs[b])), (name, b)
            assert g == int((out != cues[b]).sum()) and (out >= cues[b]).all()  # cells are set, never cleared
            grown, blocked = grown + g, blocked + k
        assert np.array_equal(cues, before)
    # the sweep exercises growing and blocking (the device test relies on this, with the same cases)
    assert grown >= 100 and blocked >= 10, (grown, blocked)


@pytest.mark.parametrize("case", dsrg_ref.handmade_cases(), ids=lambda c: c[0])
def test_handmade_cases(case):
    name, tag, cue, prob, expect = case
    out, grown, _ = dsrg_ref.seed_grow(tag, cue, prob)
    assert np.array_equal(out, expect), name
    assert np.array_equal(scan_seed_grow(tag, cue, prob), expect), name
    assert grown == int((expect != cue).sum())


def test_handmade_cases_say_what_they_claim():
    cases = {c[0]: c for c in dsrg_ref.handmade_cases()}
    _, _, cue, _, exp = cases["a-blocked-bridge"]
    assert exp[0, :, 1].tolist() == [1, 1, 0, 1, 1] and exp[0, 2, 2] == 1
    _, _, cue, _, exp = cases["c-no-row-wrap"]
    assert exp[1, 0, 1] == 0 and exp[0, 6, 1] == 1
    _, tag, cue, prob, exp = cases["d-serpentine"]
    snake = dsrg_ref.label_map(tag, prob) == 2
    lab, n = dsrg_ref.scipy.ndimage.label(snake, structure=np.ones((3, 3), int))
    assert n == 1 and int(snake.sum()) == 21 * 41 + 20 == int(exp[:, :, 1].sum())
    assert dsrg_ref.scipy.ndimage.label(snake)[1] == 1  # one pixel wide: joined through edge neighbours
    _, tag, _, prob, exp = cases["f-argmax-tie"]
    assert (dsrg_ref.label_map(tag, prob) == 3).all()  # class 2 = the first tagged class
    assert exp[1, 1, 2] == 0 and exp[:, :, 2].sum() == 19
