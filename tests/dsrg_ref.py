"""Oracle of DSRG seeded region growing (03a_sec-dsrg/DSRG.py:7-62), its input generator and hand-made cases.

The oracle is vectorised numpy + scipy.ndimage.label with a full 3 x 3 structure (8-connectivity: the reference's own
labeller, lib/CC_labeling_8.py, is not in the reference tree; label 0 = not in the class's candidate set, never filled).
tests/test_reference_pins.py holds it to what the reference's own single_generate_seed_step returned with a labeller stand-in
(tests/golden/ref_dsrg.npz; regenerate with `python oracle/gen_golden_ref.py dsrg`); tests/test_dsrg_oracle.py holds it to a per-pixel scan with its own union-find; tests/test_gpu_dsrg.py holds the device to it."""
import numpy as np
import scipy.ndimage

TH_F, TH_B = 0.5, 0.7  # DSRG.py:26


def label_map(tag, prob, th_f=TH_F, th_b=TH_B):
    """DSRG.py:28-39: 0 = no candidate class, c + 1 = candidate class c.  (H, W) int64."""
    e = np.asarray(prob, np.float32) * np.asarray(tag, np.float32).reshape(1, 1, -1)
    a = np.argmax(e, axis=2)
    is_fg = a >= 1
    fg_th = (e[:, :, 1:] > np.float32(th_f)).any(axis=2)
    bg_th = e[:, :, 0] > np.float32(th_b)
    return np.where(is_fg, fg_th, bg_th) * (a + 1)


def seed_grow(tag, cue, prob, th_f=TH_F, th_b=TH_B):
    """One image: tag (C,) or (1, 1, C), cue / prob (H, W, C) -> (new cue float32 (H, W, C), grown, blocked).
    grown = cells newly set to 1, blocked = blocked cells inside components that hold a seed.  Inputs are left alone."""
    tag = np.asarray(tag, np.float32).reshape(-1)
    cue = np.asarray(cue, np.float32)
    out = cue.copy()
    lm = label_map(tag, prob, th_f, th_b)
    one_hot = cue.sum(axis=2) == 1
    grown = blocked = 0
    for c in np.where(tag > 0.5)[0]:
        mat = lm == c + 1
        lab, _ = scipy.ndimage.label(mat, structure=np.ones((3, 3), int))
        seed = mat & (cue[:, :, c] == 1)
        hot = mat & np.isin(lab, np.unique(lab[seed]))
        stop = hot & ~seed & one_hot
        fill = hot & ~stop
        grown += int((fill & (out[:, :, c] != 1)).sum())
        blocked += int(stop.sum())
        out[fill, c] = 1
    return out, grown, blocked


def seed_grow_batch(tags, cues, probs, th_f=TH_F, th_b=TH_B):
    """-> (float32 (B, H, W, C), grown, blocked) over the batch."""
    tags = np.asarray(tags, np.float32).reshape(len(cues), -1)
    res = [seed_grow(tags[i], cues[i], probs[i], th_f, th_b) for i in range(len(cues))]
    return np.stack([r[0] for r in res]), sum(r[1] for r in res), sum(r[2] for r in res)


def make_case(rng, B, H, W, C, n_fg, normalised=True):
    """tags (B, C): background + n_fg random foreground classes per image; probs (B, H, W, C): softmax of logits that are
    constant over 6 x 6 cells (N(0, 3)) plus N(0, 0.7) per pixel plus 2 on the tagged classes -- or uniform in [0, 1) when
    not normalised; cues (B, H, W, C): Bernoulli(0.02) on the tagged classes only.  All float32."""
    tags = np.zeros((B, C), np.float32)
    tags[:, 0] = 1
    for b in range(B):
        tags[b, 1 + rng.choice(C - 1, size=min(n_fg, C - 1), replace=False)] = 1
    if normalised:
        cells = rng.normal(0, 3, (B, (H + 5) // 6, (W + 5) // 6, C))
        logits = np.repeat(np.repeat(cells, 6, axis=1), 6, axis=2)[:, :H, :W]
        logits = logits + rng.normal(0, 0.7, (B, H, W, C)) + 2 * tags[:, None, None, :]
        p = np.exp(logits - logits.max(axis=3, keepdims=True))
        probs = (p / p.sum(axis=3, keepdims=True)).astype(np.float32)
    else:
        probs = rng.random((B, H, W, C)).astype(np.float32)
    cues = ((rng.random((B, H, W, C)) < 0.02) * tags[:, None, None, :]).astype(np.float32)
    return tags, cues, probs


# (name, B, H, W, C, foreground tags, normalised): the sweep of the device test
SWEEP = [
    ("41x41x21", 4, 41, 41, 21, 3, True),
    ("5x7x3", 3, 5, 7, 3, 2, True),
    ("1x1x2", 1, 1, 1, 2, 1, True),
    ("33x65x29", 2, 33, 65, 29, 6, True),
    ("41x41x6-uniform", 2, 41, 41, 6, 3, False),
]


def sweep_cases(seed=2024):
    rng = np.random.default_rng(seed)
    return [(name,) + make_case(rng, B, H, W, C, n_fg, norm) for name, B, H, W, C, n_fg, norm in SWEEP]


def _blank(H, W, C, tag):
    """No pixel a candidate of anything (every prob 0.3: below both thresholds), no cue."""
    return np.asarray(tag, np.float32), np.zeros((H, W, C), np.float32), np.full((H, W, C), 0.3, np.float32)


def _put(prob, where, c):
    """The pixels of the boolean map `where` become candidates of class c."""
    prob[where] = 0.02
    prob[where, c] = 0.9


def handmade_cases():
    """[(name, tag (C,), cue, prob, expected new cue)] with answers known by construction."""
    cases = []

    # (a) a row of class 1, seed at column 0, a lone cue of class 2 at column 2: the blocked pixel bridges and stays
    tag, cue, prob = _blank(1, 5, 3, [0, 1, 1])
    _put(prob, np.ones((1, 5), bool), 1)
    cue[0, 0, 1] = 1
    cue[0, 2, 2] = 1
    exp = cue.copy()
    exp[0, [1, 3, 4], 1] = 1
    cases.append(("a-blocked-bridge", tag, cue, prob, exp))

    # (b) checkerboard: one colour class 1 (connected through diagonals only), the other class 2 without a seed
    tag, cue, prob = _blank(6, 7, 3, [0, 1, 1])
    yy, xx = np.mgrid[0:6, 0:7]
    even = (yy + xx) % 2 == 0
    _put(prob, even, 1)
    _put(prob, ~even, 2)
    cue[2, 4, 1] = 1
    exp = cue.copy()
    exp[even, 1] = 1
    cases.append(("b-checkerboard", tag, cue, prob, exp))

    # (c) W = 7, candidates at (0, 6) and (1, 0): consecutive linear indices, not neighbours
    tag, cue, prob = _blank(2, 7, 2, [0, 1])
    where = np.zeros((2, 7), bool)
    where[0, 6] = where[1, 0] = True
    _put(prob, where, 1)
    cue[0, 6, 1] = 1
    cases.append(("c-no-row-wrap", tag, cue, prob, cue.copy()))

    # (d) a one-pixel-wide serpentine over 41 x 41: full even rows joined at alternating ends, seed at one end
    tag, cue, prob = _blank(41, 41, 2, [1, 1])
    snake = np.zeros((41, 41), bool)
    snake[0::2] = True
    snake[1::4, 40] = True
    snake[3::4, 0] = True
    _put(prob, snake, 1)
    cue[0, 0, 1] = 1
    exp = cue.copy()
    exp[snake, 1] = 1
    cases.append(("d-serpentine", tag, cue, prob, exp))

    # (e) nothing tagged / nothing seeded: the cues come back as they went in
    tag, cue, prob = _blank(5, 6, 3, [0, 0, 0])
    _put(prob, np.ones((5, 6), bool), 1)
    cue[1, 1, 1] = cue[3, 2, 2] = 1
    cases.append(("e-no-tags", tag, cue, prob, cue.copy()))
    tag, cue, prob = _blank(5, 6, 3, [1, 1, 1])
    _put(prob, np.ones((5, 6), bool), 1)
    cases.append(("e-no-seeds", tag, cue, prob, cue.copy()))

    # (f) background untagged, prob constant over the classes: the first TAGGED class wins the arg-max tie everywhere;
    # the lone cue of class 3 sits on a class-2 pixel and blocks it
    tag, cue, prob = _blank(4, 5, 4, [0, 0, 1, 1])
    prob[:] = 0.6
    cue[0, 0, 2] = 1
    cue[1, 1, 3] = 1
    exp = cue.copy()
    exp[:, :, 2] = 1
    exp[1, 1, 2] = 0
    cases.append(("f-argmax-tie", tag, cue, prob, exp))
    return cases
