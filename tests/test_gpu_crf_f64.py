"""GPU: the dense-CRF mean-field loop (wsc_crf_*, wsc_crf_v_*) against a float64 evaluation of the oracle's lattice, per pixel.

The reference is helpers.crf_oracle64: oracle/densecrf_ref.c built with -DCRF_F64 -- the fp32 oracle's own vertex ids, neighbour
tables and barycentric weights, every value from the splat down in double.  Bounds are multiples of the fp32 C oracle's OWN
distance to that reference (helpers.D32_ONE_STEP, recorded from and re-checked by the CPU tests of tests/test_crf_oracle.py;
per case in the product regime), never of anything the device gave:

  one iteration, product compatibilities         max|Q - Q64| <= 4 x D32_ONE_STEP
  ten iterations, contractive compatibilities    max|Q - Q64| <= 4 x D32_ONE_STEP
  product regime (10 / 10 / 5 iterations)        max|Q - Q64| <= 8 x max(d32 of the case, D32_ONE_STEP)

4 x: the device and the C oracle are two fp32 evaluations with different summation orders (2 x between two orders alone in
DESIGN.md section 5's conv table), the device adds v_exp_f32 / v_rcp_f32 at about 1 ulp each and the 2^-24 quantisation of its
slot partials.  8 x: in the product regime the error is conditioning x per-step noise, and d32 is ONE realisation of it.
Labels: every pixel whose float64 top-two margin exceeds 2 x the bound carries the float64 label -- no share is excused -- and
the pixels below that margin are at most 1 % of an image.

Every case runs twice on a context of its own: the first use of an image size takes the blur-kernel path for the Gaussian
lattice, the second forms that message on chip (where the size's tile vertex sets fit); both runs are held to the bound.
Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

from tests import crf_f64_cases as f64c
from tests import helpers
from wsscam import _lib

pytestmark = pytest.mark.gpu

_ids = lambda c: c.name  # noqa: E731


def _device_run(ctx, case, labels_only=False):
    """One call through the C ABI.  Returns ([Q (M, N) per image] or None, [labels (N,)], [(V_g, V_b)] or None, on_chip or None)."""
    g_sxy, g_compat, bi_sxy, bi_srgb, bi_compat, n_iters = case.cfg
    images = case.images
    bufs = []

    def dev(a):
        bufs.append(ctx.to_device(np.ascontiguousarray(a)))
        return bufs[-1]

    def alloc(n):
        bufs.append(ctx.alloc(n))
        return bufs[-1]

    try:
        if case.kind == "ragged":
            sizes = [im[0].shape[:2] for im in images]
            Ms = [im[1].shape[0] for im in images]
            cv = _lib.CrfV(ctx, [dev(im[0]) for im in images], sizes, g_sxy, bi_sxy, bi_srgb)
            q_devs = None if labels_only else [alloc(m * h * w * 4) for (h, w), m in zip(sizes, Ms)]
            a_devs = [alloc(h * w * 4) for (h, w) in sizes]
            cv.inference([dev(im[1]) for im in images], Ms, g_compat, bi_compat, n_iters, q_devs, a_devs)
            qs = None if labels_only else [ctx.to_host(q, (m, h * w), np.float32) for q, (h, w), m in zip(q_devs, sizes, Ms)]
            labs = [ctx.to_host(a, (h * w,), np.int32) for a, (h, w) in zip(a_devs, sizes)]
            cv.close()
            return qs, labs, None, None
        B = len(images)
        H, W, _ = images[0][0].shape
        M, N = images[0][1].shape[0], H * W
        U = np.stack([im[1] for im in images])
        if case.kind == "pm":  # [B][N][Mp], Mp = 4 ceil(M / 4), padding columns zero: wsc_cam_unary_pm's layout
            Mp = (M + 3) // 4 * 4
            Upm = np.zeros((B, N, Mp), np.float32)
            Upm[:, :, :M] = np.transpose(U, (0, 2, 1))
            U = Upm
        crf = _lib.Crf(ctx, dev(np.stack([im[0] for im in images])), B, H, W, g_sxy, bi_sxy, bi_srgb)
        vg, vb = crf.lattice_sizes()
        on_chip = crf.gaussian_on_chip(M)
        q_dev = None if labels_only else alloc(B * M * N * 4)
        a_dev = alloc(B * N * 4)
        crf.inference(dev(U), M, g_compat, bi_compat, n_iters, q_dev, a_dev, pixel_major=case.kind == "pm")
        q = None if labels_only else list(ctx.to_host(q_dev, (B, M, N), np.float32))
        labs = list(ctx.to_host(a_dev, (B, N), np.int32))
        crf.close()
        return q, labs, [(int(g), int(b)) for g, b in zip(vg, vb)], on_chip
    finally:
        for b in bufs:
            b.free()


def _expect_on_chip(case):
    """Second use of a size: True where tests/test_gpu_crf.py pins the on-chip message (g_sxy >= 1; of the narrow kernels its
    9 x 7 image, whose tile vertex sets fit the LDS), None where it makes no claim (the other narrow-kernel sizes legitimately
    stay off chip at larger M; a ragged batch has no query)."""
    if case.kind == "ragged":
        return None
    if case.cfg[0] >= 1.0 or case.name.startswith("gsxy0.25-9x7"):
        return True
    return None


def _check(regime, case, labels_only_too=False):
    refs = [helpers.crf_oracle64(rgb, U, case.cfg) for rgb, U in case.images]
    d32 = None
    if regime == "product":  # the fp32 oracle's own distance on this case, computed here on the CPU
        d32 = max(float(np.abs(helpers.crf_oracle(rgb, U, case.cfg)[0] - r[0]).max()) for (rgb, U), r in zip(case.images, refs))
    bound = f64c.bound_of(regime, case, d32)
    ok = [f64c.decided(r[0], bound) for r in refs]
    undecided = max(1 - float(o.mean()) for o in ok)
    ctx = _lib.Context(0)
    failures = []
    try:
        dists, chips = [], []
        for run in (0, 1):
            qs, labs, sizes, on_chip = _device_run(ctx, case)
            chips.append(on_chip)
            dists.append(max(float(np.abs(q.astype(np.float64) - r[0]).max()) for q, r in zip(qs, refs)))
            for i, (q, lab, r, o) in enumerate(zip(qs, labs, refs, ok)):
                if sizes is not None and sizes[i] != (int(r[2][0]), int(r[2][1])):
                    failures.append("run %d image %d: lattice sizes %s, oracle %s" % (run, i, sizes[i], tuple(r[2])))
                wrong = int((lab[o] != r[1][o]).sum())
                if wrong:
                    failures.append("run %d image %d: %d decided pixels do not carry the float64 label" % (run, i, wrong))
                if not np.array_equal(lab, q.argmax(0)):
                    failures.append("run %d image %d: labels are not the arg-max of Q" % (run, i))
        labels_only_wrong = None
        if labels_only_too:
            _, labs, _, _ = _device_run(ctx, case, labels_only=True)
            labels_only_wrong = sum(int((lab[o] != r[1][o]).sum()) for lab, r, o in zip(labs, refs, ok))
            if labels_only_wrong:
                failures.append("labels-only call: %d decided pixels do not carry the float64 label" % labels_only_wrong)
    finally:
        ctx.close()
    print("\n[crf-f64] %-11s %-34s d32 = %s  device = %.3e (blur kernels) %.3e (2nd use, on chip: %s)  bound = %.3e  "
          "device/bound = %.2f  undecided = %.4f%s%s" %
          (regime, case.name, "%.3e" % d32 if d32 is not None else "%.1e*" % f64c.d32_recorded(case), dists[0], dists[1], chips[1],
           bound, max(dists) / bound, undecided, "" if labels_only_wrong is None else "  labels-only wrong = %d" % labels_only_wrong,
           "  ILL-CONDITIONED (d32 > 1e-4)" if d32 is not None and d32 > 1e-4 else ""))
    assert undecided <= 0.01, undecided
    if case.kind != "ragged":
        assert chips[0] is False, "first use of a size must take the blur-kernel path"
        if _expect_on_chip(case):
            assert chips[1] is True, "second use of this size must form the Gaussian message on chip"
    assert dists[0] <= bound, ("blur-kernel path", dists[0], bound)
    assert dists[1] <= bound, ("second use", dists[1], bound)
    assert not failures, failures


@pytest.mark.parametrize("case", f64c.one_step_cases(), ids=_ids)
def test_crf_one_iteration_vs_float64(built, case):
    """(a) One iteration with the product's compatibilities (3, 10): lattice build, splat, all blur paths, slice, message and
    soft-max once, nothing amplified.  Bound 4 x D32_ONE_STEP.  The three configurations x M in {1, 2, 3, 6, 21, 29, 32} at
    57 x 75 in batches of 3, 321 x 321 M = 21, 281 x 500 with label unaries, the flat and the uniform-noise image, g_sxy = 0.25
    and 5, the degenerate sizes, the pixel-major entry (M = 21 -> Mp = 24, M = 8) and one ragged batch."""
    _check("one_step", case)


@pytest.mark.parametrize("case", f64c.contractive_cases(), ids=_ids)
def test_crf_ten_contractive_iterations_vs_float64(built, case):
    """(b) Ten iterations with compatibilities (1, 2), under which the iteration damps rounding (the fp32 oracle stays at its
    one-step distance): every iteration's kernels -- the first, the middle ones, the last with its Q / arg-max output -- at
    the one-step bound, sharp = 3 and sharp = 10 unaries included, and the labels-only call (q_dev = NULL)."""
    _check("contractive", case, labels_only_too=True)


@pytest.mark.parametrize("case", f64c.product_cases(), ids=_ids)
def test_crf_product_regime_vs_float64(built, case):
    """(c) The product's compatibilities at 10 / 10 / 5 iterations on the inputs of test_crf_vs_oracle, test_crf_321_config3,
    test_crf_random_sweep and test_crf_config5_sizes.  Rounding is amplified here (3-5 x per iteration on some inputs), so the
    bound follows the fp32 oracle's own distance on the case: 8 x max(d32, D32_ONE_STEP); a case with d32 > 1e-4 is printed as
    ill-conditioned (sweep7) and kept."""
    _check("product", case)
