"""Case lists of the float64 pin of the dense-CRF mean-field loop, shared by tests/test_crf_oracle.py (CPU: the fp32 C oracle
against helpers.crf_oracle64) and tests/test_gpu_crf_f64.py (the device against helpers.crf_oracle64).

Three regimes:
  one_step_cases()     one iteration, product compatibilities (3, 10): every kernel of an iteration, no amplification
  contractive_cases()  ten iterations with compatibilities (1, 2): the iteration damps rounding, so every iteration's kernels
                       are held to the one-step bound
  product_cases()      10 / 10 / 5 iterations with the product's compatibilities: rounding is amplified 3-5 x per step on some
                       inputs, the bound follows the fp32 oracle's own distance per case

A case is Case(name, kind, images, cfg): images = [(rgb uint8 (H, W, 3), U float32 (M, H*W))] (or a function that makes them:
the lists are cheap to build, an image is drawn when a test first asks), cfg = (g_sxy, g_compat, bi_sxy, bi_srgb, bi_compat,
n_iters); kind "batch" (one wsc_crf over equal-size, equal-M images), "pm" (the same through the
pixel-major entry) or "ragged" (one wsc_crf_v over images of their own sizes and class counts).

    python -m tests.crf_f64_cases            prints max|Q32 - Q64| per case and the maxima D32_ONE_STEP is set from
    python -m tests.crf_f64_cases --sharp    the sharp = 10 seed search behind SHARP10_SEED
"""
import functools
import os
import sys

import numpy as np

from tests import helpers

_PKG = os.path.join(helpers.ROOT, "wsss-analysis_amd")  # (python -m tests.crf_f64_cases runs without tests/conftest.py)
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)



class Case:
    def __init__(self, name, kind, images, cfg):
        self.name, self.kind, self.cfg = name, kind, tuple(cfg)
        self._images = images

    @property
    def images(self):
        if callable(self._images):
            self._images = self._images()
        return self._images

    def __repr__(self):
        return "Case(%s, %s)" % (self.name, self.cfg)


# (g_sxy, g_compat, bi_sxy, bi_srgb, bi_compat, n_iters): tests/test_gpu_crf.py::CFGS
CFGS = [(1.5, 3, 40, 13, 10, 10), (3, 3, 50, 5, 10, 10), (3 / 12, 3, 80 / 12, 13, 10, 5)]
CONTRACTIVE = (1, 2)  # (g_compat, bi_compat) under which the mean-field iteration damps rounding instead of amplifying it

# synth_crf_case(sharp=10) under the product compatibilities (3, 10), 10 iterations, narrow bilateral kernel (sxy 6, srgb 1.5):
# bistable pixels, where the fp32 oracle ITSELF is 1.9e-2 from the float64 evaluation of its own lattice.  Worst of seeds 0..29
# x 6 kernel-width sets x M in 2..5 x three small sizes (--sharp prints the seeds of this one), see
# tests/test_crf_oracle.py::test_fp32_parity_1e3_is_false_on_sharp_unaries.
SHARP10_SEED = 9
SHARP10_SHAPE = (57, 75, 3)
SHARP10_CFG = (3, 3, 6, 1.5, 10, 10)


def _with(cfg, compats=None, iters=None):
    g, b = (cfg[1], cfg[4]) if compats is None else compats
    return (cfg[0], g, cfg[2], cfg[3], b, cfg[5] if iters is None else iters)


def _synth_now(seed, H, W, M, B, sharp=3.0):
    rng = np.random.default_rng(seed)
    return [helpers.synth_crf_case(rng, H, W, M, sharp=sharp)[:2] for _ in range(B)]


def _synth(*args, **kw):
    return functools.partial(_synth_now, *args, **kw)


def _label_unary_image_now(seed, H, W, M):
    from wsscam.misc import imutils

    rng = np.random.default_rng(seed)
    rgb, _, p = helpers.synth_crf_case(rng, H, W, M)
    return [(rgb, np.ascontiguousarray(imutils.unary_from_labels(p.argmax(0), M, 0.7, zero_unsure=False)))]


def _label_unary_image(*args):
    return functools.partial(_label_unary_image_now, *args)


def _flat_image():
    """tests/test_gpu_crf.py::test_crf_flat_image_long_rows: thousands of pixels on one bilateral vertex."""
    H, W, M = 96, 96, 3
    _, U, _ = helpers.synth_crf_case(np.random.default_rng(12), H, W, M)
    return [(np.full((H, W, 3), 200, np.uint8), U)]


def _noise_image():
    """tests/test_gpu_edge.py::test_crf_noise_image_hash_table_fallback: more bilateral vertices than pixels."""
    rng = np.random.default_rng(41)
    H, W, M = 64, 72, 3
    noise = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    _, U, _ = helpers.synth_crf_case(rng, H, W, M)
    return [(noise, U)]


def _degenerate(shape):
    """tests/test_gpu_edge.py::test_crf_degenerate_sizes."""
    rng = np.random.default_rng(4)
    H, W = shape
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    p = rng.random((3, H * W)).astype(np.float32) + 0.05
    return [(rgb, np.ascontiguousarray(-np.log(p / p.sum(0, keepdims=True))))]


RAGGED_SPECS = [(57, 75, 3), (40, 33, 21), (57, 75, 6), (64, 64, 2), (57, 75, 1), (40, 33, 5), (57, 75, 21)]


def _ragged():
    rng = np.random.default_rng(4711)
    return [helpers.synth_crf_case(rng, h, w, m)[:2] for (h, w, m) in RAGGED_SPECS]


def _shape_cases(Ms, compats, iters, big=True):
    """The shapes of the one-step list; Ms thins the 57 x 75 block.  iters = None keeps each configuration's own count."""
    out = []
    for ci, cfg in enumerate(CFGS):
        for M in Ms:
            out.append(Case("cfg%d-M%d-57x75x3" % (ci, M), "batch", _synth(100 + M, 57, 75, M, 3), _with(cfg, compats, iters)))
    if big:
        out.append(Case("321x321-M21", "batch", _synth(7, 321, 321, 21, 1), _with(CFGS[0], compats, iters)))
        out.append(Case("281x500-M3-label-unaries", "batch", _label_unary_image(5, 281, 500, 3), _with(CFGS[1], compats, iters)))
    out.append(Case("flat-96x96-M3", "batch", _flat_image, _with((3, 3, 80, 13, 10, 5), compats, iters)))
    out.append(Case("noise-64x72-M3", "batch", _noise_image, _with((3, 3, 50, 5, 10, 3), compats, iters)))
    out.append(Case("gsxy5-33x200-M29", "batch", _synth(33 * 7 + 200, 33, 200, 29, 1), _with((5, 3, 40, 13, 10, 2), compats, iters)))
    out.append(Case("gsxy0.25-9x7-M2", "batch", _synth(9 * 7 + 7, 9, 7, 2, 1), _with(CFGS[2], compats, iters)))
    out.append(Case("gsxy0.25-41x41-M21x2", "batch", _synth(71, 41, 41, 21, 2), _with(CFGS[2], compats, iters)))
    for shape in [(1, 1), (1, 37), (29, 1), (3, 5)]:
        out.append(Case("degenerate-%dx%d" % shape, "batch", functools.partial(_degenerate, shape), _with(CFGS[0], compats, iters)))
    out.append(Case("pixel-major-M21-45x45x2", "pm", _synth(41, 45, 45, 21, 2), _with(CFGS[0], compats, iters)))
    out.append(Case("pixel-major-M8-32x32", "pm", _synth(42, 32, 32, 8, 1), _with(CFGS[0], compats, iters)))
    out.append(Case("ragged-7-images", "ragged", _ragged, _with(CFGS[0], compats, iters)))
    return out


def one_step_cases():
    return _shape_cases([1, 2, 3, 6, 21, 29, 32], None, 1)


def contractive_cases():
    out = _shape_cases([1, 3, 21, 32], CONTRACTIVE, 10)
    for sharp in (3, 10):
        for ci in (0, 1):
            out.append(Case("sharp%d-cfg%d-M6-57x75x2" % (sharp, ci), "batch", _synth(200 + sharp, 57, 75, 6, 2, sharp=float(sharp)),
                            _with(CFGS[ci], CONTRACTIVE, 10)))
    return out


def product_cases(large=True):
    """The inputs of test_crf_vs_oracle, test_crf_321_config3, test_crf_random_sweep and test_crf_config5_sizes, as those tests
    draw them.  large = False leaves out 1088 x 1088 (ten CPU-seconds per oracle run)."""
    out = []
    for ci, cfg in enumerate(CFGS):
        for M in [1, 2, 3, 6, 21, 32]:
            out.append(Case("vs_oracle-cfg%d-M%d" % (ci, M), "batch", _synth(100 + M, 57, 75, M, 3), cfg))
    out.append(Case("321_config3", "batch", _synth(7, 321, 321, 21, 1), CFGS[0]))
    rng = np.random.default_rng(77)
    for it in range(10):
        H, W = int(rng.integers(5, 90)), int(rng.integers(5, 90))
        M = int(rng.integers(1, 33))
        B = int(rng.integers(1, 5))
        cfg = CFGS[it % len(CFGS)][:5] + (int(rng.integers(1, 11)),)
        images = [helpers.synth_crf_case(rng, H, W, M)[:2] for _ in range(B)]
        out.append(Case("sweep%d-%dx%dx%d-M%d-%dit" % (it, H, W, B, M, cfg[5]), "batch", images, cfg))
    sizes = [(321, 321, 29, CFGS[0]), (41, 41, 21, CFGS[2])] + ([(1088, 1088, 5, CFGS[0])] if large else [])
    for (H, W, M, cfg) in sizes:
        out.append(Case("config5-%dx%d-M%d" % (H, W, M), "batch", _synth(50 + M, H, W, M, 1), cfg))
    return out


def sharp10_case():
    H, W, M = SHARP10_SHAPE
    return Case("sharp10-seed%s" % SHARP10_SEED, "batch", _synth(SHARP10_SEED, H, W, M, 1, sharp=10.0), SHARP10_CFG)


def oracle_pair(case):
    """[(Q32, labels32, Q64, labels64, sizes32, sizes64)] per image of a case."""
    out = []
    for rgb, U in case.images:
        q32, a32, l32 = helpers.crf_oracle(rgb, U, case.cfg)
        q64, a64, l64 = helpers.crf_oracle64(rgb, U, case.cfg)
        out.append((q32, a32, q64, a64, l32, l64))
    return out


def d32_of(pairs):
    return max(float(np.abs(p[0] - p[2]).max()) for p in pairs)


def d32_recorded(case):
    """The recorded fp32-oracle distance a one-step / contractive case is held to (helpers.D32_ONE_STEP; the flat image, whose
    oracle sums are thousands of terms long, helpers.D32_LONG_ROWS)."""
    return helpers.D32_LONG_ROWS if case.name.startswith("flat-") else helpers.D32_ONE_STEP


def bound_of(regime, case, d32=None):
    """The device's bound on max|Q - Q64|: 4 x the recorded one-step distance where nothing amplifies rounding; in the product
    regime 8 x the fp32 oracle's own distance on that case (never below the one-step distance)."""
    if regime == "product":
        return 8 * max(d32, helpers.D32_ONE_STEP)
    return 4 * d32_recorded(case)


def decided(q64, bound):
    """Pixels whose float64 top-two margin exceeds 2 x bound: two results within `bound` of Q64 cannot disagree on their label."""
    return helpers.top2_margin(q64) > 2 * bound


REGIMES = {"one_step": one_step_cases, "contractive": contractive_cases, "product": product_cases}


def _main(argv):
    if "--sharp" in argv:
        H, W, M = SHARP10_SHAPE
        for seed in range(30):
            c = Case("sharp10", "batch", _synth(seed, H, W, M, 1, sharp=10.0), SHARP10_CFG)
            print("sharp = 10 seed %2d: max|Q32 - Q64| = %.3e" % (seed, d32_of(oracle_pair(c))))
        return
    worst = {}
    for regime, cases in REGIMES.items():
        for c in cases():
            pairs = oracle_pair(c)
            d32 = d32_of(pairs)
            bound = bound_of(regime, c, d32)
            share = max(1 - float(decided(p[2], bound).mean()) for p in pairs)
            flips = sum(int(((p[1] != p[3]) & decided(p[2], bound)).sum()) for p in pairs)
            print("%-12s %-34s d32 = %.3e  bound = %.3e  undecided <= %.4f  flips on decided pixels = %d" %
                  (regime, c.name, d32, bound, share, flips))
            key = regime + (" (flat image)" if c.name.startswith("flat-") else "")
            worst[key] = max(worst.get(key, 0.0), d32)
    print("worst:", {k: "%.3e" % v for k, v in worst.items()})


if __name__ == "__main__":
    _main(sys.argv[1:])
