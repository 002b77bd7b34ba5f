"""Oracle of the 02_cues localization seeds (02_cues/utilities.py:183-278, 02_cues/adp_cues.py:304-339), its input generator
and hand-made cases.

The oracle is the per-pixel statement of include/wsscam.h (wsc_cue_seeds), vectorised over pixels:
  foreground mask   float64(fg) > thresh * float64(max), max over the batch or over the image's own map
  background mask   sequential float64 sum over the channels, 3 x 3 median (numpy 'symmetric' pad = scipy's 'reflect', a sort
                    of the nine window values), strictly below the value of rank int(bg_fraction * H * W)
  label             k + 1 for the covering channel k of the smallest area, the HIGHER index among equal areas
                    (= painting from the largest to the smallest mask under np.argsort(-area, kind='stable')), 0 if uncovered
A pixel is AMBIGUOUS when its smallest covering area is shared by two or more covering masks: there the reference's own
np.argsort(-area) (default kind, unspecified order among ties) may paint either way.
tests/test_reference_pins.py holds the oracle, on every other pixel, to the labels that the reference's own get_fgbg_cues / get_fg_cues /
update_cues returned (tests/golden/ref_cue_seeds.npz; regenerate with `python oracle/gen_golden_ref.py cue_seeds`);
tests/test_cue_seeds_oracle.py holds the oracle to the host functions of wsscam.cues.utilities on every other pixel;
tests/test_gpu_cue_seeds.py holds the device to the oracle on every pixel."""
import numpy as np

BG_FRACTION = 0.1  # utilities.py:203: int(0.1 * H * W)


def sequential_sum(stack):
    """sum_k float64(stack[k]) added one channel after the other, from channel 0."""
    s = np.array(stack[0], dtype=np.float64)
    for k in range(1, len(stack)):
        s = s + np.asarray(stack[k], dtype=np.float64)
    return s


def median3x3(plane):
    """scipy.ndimage.median_filter(plane, 3) with its default mode='reflect': the edge sample is repeated."""
    H, W = plane.shape
    p = np.pad(plane, 1, mode="symmetric")
    win = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=-1)
    return np.sort(win, axis=-1)[..., 4]


def background_mask(bg, bg_fraction=BG_FRACTION):
    """bg (Cb, H, W) -> bool (H, W)."""
    med = median3x3(sequential_sum(bg))
    k = int(bg_fraction * med.shape[0] * med.shape[1])
    return med < np.partition(med.ravel(), k)[k]


def masks(fg, bg, thresh, per_image_max=False, bg_fraction=BG_FRACTION):
    """fg (B, C, H, W), bg (B, Cb, H, W) or None -> bool (B, L, H, W), channel 0 the background when bg is given."""
    f = np.asarray(fg, dtype=np.float64)
    mx = f.max(axis=(2, 3)) if per_image_max else np.broadcast_to(f.max(axis=(0, 2, 3)), f.shape[:2])
    m = f > (thresh * mx)[:, :, None, None]
    if bg is None:
        return m
    b = np.stack([background_mask(x, bg_fraction) for x in bg])
    return np.concatenate([b[:, None], m], axis=1)


def resolve(m):
    """bool (B, L, H, W) -> (labels uint8 (B, H, W), areas int32 (B, L), ambiguous bool (B, H, W))."""
    B, L, H, W = m.shape
    area = m.sum(axis=(2, 3)).astype(np.int64)
    big = np.where(m, area[:, :, None, None], np.iinfo(np.int64).max)
    hit = m & (big == big.min(axis=1, keepdims=True))  # the covering channels of the smallest area
    top = L - 1 - np.argmax(hit[:, ::-1], axis=1)      # the highest of them
    labels = np.where(m.any(axis=1), top + 1, 0).astype(np.uint8)
    return labels, area.astype(np.int32), hit.sum(axis=1) >= 2


def seeds(fg, bg, thresh, per_image_max=False, bg_fraction=BG_FRACTION):
    """-> (labels uint8 (B, H, W), areas int32 (B, L), ambiguous bool (B, H, W))."""
    return resolve(masks(fg, bg, thresh, per_image_max, bg_fraction))


def labels_from_cues(cues, indices, H, W):
    """The `'%d_cues'` arrays (class, row, col) of a cue dict as label maps: int64 (B, H, W), class + 1, 0 = none."""
    out = np.zeros((len(indices), H, W), np.int64)
    for i, x in enumerate(indices):
        c = np.asarray(cues["%d_cues" % x])
        out[i, c[1], c[2]] = c[0] + 1
    return out


# ---- the sweep ---------------------------------------------------------------------------------------------------------
SHAPES = [(2, 20, 20, 41, 41),  # the VOC size
          (3, 5, 2, 7, 6),
          (1, 31, 0, 41, 41),   # foreground only at L = 31
          (4, 3, 1, 64, 64),    # the pixel limit
          (2, 31, 3, 3, 37),
          (2, 8, 2, 33, 65),
          (1, 1, 1, 1, 1)]      # (B, C, Cb, H, W); Cb = 0: no background stack
SEEDS = [1000, 1001, 1002, 1003, 1004]
SWEEP = [("%dx%dx%dx%dx%d-%d" % (shape + (seed,)), shape, seed) for shape in SHAPES for seed in SEEDS]


def _stack(rng, B, C, H, W):
    """Cubed uniforms (a few strong responses over a low floor), about half of the (b, c) maps zeroed as gated classes are."""
    x = (rng.random((B, C, H, W)) ** 3).astype(np.float32)
    x[rng.random((B, C)) < 0.5] = 0
    return x


def make_case(shape, seed):
    """-> (fg float32 (B, C, H, W), bg float32 (B, Cb, H, W) or None)."""
    B, C, Cb, H, W = shape
    rng = np.random.default_rng(seed)
    fg = _stack(rng, B, C, H, W)
    return fg, (_stack(rng, B, Cb, H, W) if Cb else None)


def sweep_cases():
    return [(name,) + make_case(shape, seed) for name, shape, seed in SWEEP]


# ---- hand-made cases ---------------------------------------------------------------------------------------------------
def threshold_neighbours(thresh=0.2, top=0.7):
    """A (1, 1, 1, 4) map [top, lo, hi, 0] with lo / hi the two float32 neighbours of thresh * top formed in double: only hi is
    a seed.  `top` is chosen so that the float32 product rounds UP to hi -- a float32 `x > thresh * max` drops hi."""
    t = thresh * float(np.float32(top))
    hi = np.float32(t)
    if float(hi) <= t:
        hi = np.nextafter(hi, np.float32(np.inf))
    lo = np.nextafter(hi, np.float32(-np.inf))
    assert float(lo) <= t < float(hi)
    t32 = np.float32(thresh) * np.float32(top)
    assert (lo > t32) == (hi > t32), "a float32 product must put both neighbours on one side"
    return np.array([top, lo, hi, 0], np.float32).reshape(1, 1, 1, 4)


def rank_order_channels():
    """Background channels (1, 3, 4, 4) on which the float32 sum and the reversed-order double sum rank a different pixel at
    k = int(0.5 * 16) = 8 than the sequential double sum does.  The planes are constant along rows, so a row's medians are the
    median of its own and its neighbours' sums (the first and the last row: their own)."""
    big60, big30 = np.float32(2.0 ** 60), np.float32(2.0 ** 30)
    rows = [(3, 0, 0),            # every order and format: 3
            (1, 0, 0),            # 1
            (big60, -big60, 5),   # sequential double and float32: 5;  reversed: (5 - 2^60) + 2^60 = 0
            (big30, 7, -big30)]   # either double order: 7;  float32: 2^30 + 7 rounds to 2^30, so 0
    bg = np.zeros((1, 3, 4, 4), np.float32)
    for y, row in enumerate(rows):
        for k, v in enumerate(row):
            bg[0, k, y, :] = v

    def mask(plane):
        med = median3x3(np.asarray(plane, np.float64))
        return med < np.partition(med.ravel(), 8)[8]

    seq = background_mask(bg[0], 0.5)
    assert seq.any() and np.array_equal(seq, mask(sequential_sum(bg[0])))
    assert not np.array_equal(mask((bg[0, 0] + bg[0, 1]) + bg[0, 2]), seq), "the float32 sum must rank another pixel"
    assert not np.array_equal(mask(sequential_sum(bg[0, ::-1])), seq), "the reversed-order sum must rank another pixel"
    return bg


def border_plane():
    """A plane that differs from 1 on its border only, on which the seeds under scipy's 'reflect' border (rank k = 3) differ
    from those under a constant, a 'mirror' or a 'wrap' border."""
    return np.array([[1, 0, 0, 0, 0, 2],
                     [1, 1, 1, 1, 1, 1],
                     [2, 1, 1, 1, 1, 2],
                     [2, 1, 1, 1, 1, 2],
                     [2, 1, 1, 1, 1, 1],
                     [1, 1, 0, 1, 2, 1]], np.float32).reshape(1, 1, 6, 6)


def handmade_cases():
    """[(name, fg, bg or None, kwargs of seeds(), expected labels (B, H, W) or None)]: answers known by construction where given;
    every case is also compared with the oracle."""
    cases = []

    fg = threshold_neighbours()
    cases.append(("threshold-neighbours", fg, None, dict(thresh=0.2), np.array([[[1, 0, 1, 0]]])))

    # Q7: image 0 scaled by 10 moves image 1's threshold in batch scope only
    k = np.arange(1, 21, dtype=np.float32).reshape(4, 5)
    base = (k * np.float32(0.0625)).reshape(1, 1, 4, 5)  # max 1.25: seeds where k / 16 > 0.25
    fg = np.concatenate([base * 10, base])                # batch max 12.5: image 1 has nothing above 2.5
    on = (k >= 5).astype(np.uint8)
    cases.append(("batch-scope", fg, None, dict(thresh=0.2, per_image_max=False), np.stack([on, np.zeros_like(on)])))
    cases.append(("image-scope", fg, None, dict(thresh=0.2, per_image_max=True), np.stack([on, on])))

    # a class gated to zero between two live ones
    fg = np.zeros((1, 3, 3, 3), np.float32)
    fg[0, 0, 0, :] = 1
    fg[0, 2, 2, :] = 1
    cases.append(("gated-class", fg, None, dict(thresh=0.2), np.array([[[1, 1, 1], [0, 0, 0], [3, 3, 3]]])))

    # an all-negative map in image scope: thresh * max is negative, everything above it is a seed
    fg = -np.arange(1, 10, dtype=np.float32).reshape(1, 1, 3, 3)  # max = -1: seeds where v > -0.5 -- nowhere
    cases.append(("all-negative-none", fg, None, dict(thresh=0.5, per_image_max=True), np.zeros((1, 3, 3), np.uint8)))
    cases.append(("all-negative-some", fg, None, dict(thresh=3.5, per_image_max=True),  # v > -3.5: -1, -2, -3
                  np.array([[[1, 1, 1], [0, 0, 0], [0, 0, 0]]])))

    # a constant background plane: nothing is strictly below the rank-k value
    fg = np.zeros((1, 1, 5, 5), np.float32)
    fg[0, 0, 2, 2] = 1
    lab = np.zeros((1, 5, 5), np.uint8)
    lab[0, 2, 2] = 2
    cases.append(("constant-background", fg, np.full((1, 2, 5, 5), 0.25, np.float32), dict(thresh=0.2), lab))

    # many medians equal the rank-k value: rows 0-1 hold 0, the rest 1; k = int(0.1 * 100) = 10 lands among the twenty zeros
    bg = np.ones((1, 1, 10, 10), np.float32)
    bg[0, 0, :2] = 0
    cases.append(("rank-value-repeated", np.zeros((1, 1, 10, 10), np.float32), bg, dict(thresh=0.2), np.zeros((1, 10, 10), np.uint8)))
    # ... and with k among the ones (bg_fraction 0.5: k = 50) the twenty zeros are all strictly below
    lab = np.zeros((1, 10, 10), np.uint8)
    lab[0, :2] = 1
    cases.append(("rank-value-above", np.zeros((1, 1, 10, 10), np.float32), bg, dict(thresh=0.2, bg_fraction=0.5), lab))

    cases.append(("sum-order", np.zeros((1, 1, 4, 4), np.float32), rank_order_channels(), dict(thresh=0.2, bg_fraction=0.5), None))

    lab = np.zeros((1, 6, 6), np.uint8)
    lab[0, 0, 2:4] = 1
    cases.append(("reflect-border", np.zeros((1, 1, 6, 6), np.float32), border_plane(), dict(thresh=0.2), lab))

    # two overlapping masks of equal area: the higher index wins the overlap
    fg = np.zeros((1, 2, 4, 4), np.float32)
    fg[0, 0, :2, :] = 1   # rows 0-1: 8 pixels
    fg[0, 1, 1:3, :] = 1  # rows 1-2: 8 pixels
    cases.append(("equal-areas", fg, None, dict(thresh=0.2), np.array([[[1] * 4, [2] * 4, [2] * 4, [0] * 4]])))

    # nested masks of three sizes: the smallest covering mask shows
    fg = np.zeros((1, 3, 7, 7), np.float32)
    fg[0, 1] = 1              # 49
    fg[0, 2, 1:6, 1:6] = 1    # 25
    fg[0, 0, 2:5, 2:5] = 1    # 9
    lab = np.full((1, 7, 7), 2, np.uint8)
    lab[0, 1:6, 1:6] = 3
    lab[0, 2:5, 2:5] = 1
    cases.append(("nested", fg, None, dict(thresh=0.2), lab))

    # bg_fraction = 0: the rank-0 value is the minimum, nothing is below it
    rng = np.random.default_rng(7)
    fg = _stack(rng, 1, 2, 6, 5)
    cases.append(("fraction-zero", fg, _stack(rng, 1, 3, 6, 5) + np.float32(0.1), dict(thresh=0.2, bg_fraction=0.0), None))
    return cases
