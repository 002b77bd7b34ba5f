"""GPU: the 01_train sample transform on the device (csrc/cls_batch.hip, wsc_cls_train_batch) against tests/cls_batch_ref.py, the
numpy restatement tests/test_cls_batch_oracle.py pins against PIL and scipy themselves.  Every comparison is an equality of bits.

The packed images and the output lie between 4 KiB of sentinel bytes, which must be intact afterwards; a refused call must leave
the output's sentinels in place as well (nothing was launched)."""
import ctypes

import numpy as np
import pytest

from tests import cls_batch_ref as ref
from tests.test_gpu_irn_batch import SENTINEL, Guarded, _pack
from wsscam import _lib

pytestmark = pytest.mark.gpu

MODES = ("nearest", "reflect", "constant")
DATASETS = ("ADP", "VOC2012", "DeepGlobe")
MIXED_FLAGS = (ref.FLAG_WARP, ref.FLAG_WARP | ref.FLAG_FLIP_COLS, ref.FLAG_FLIP_ROWS, ref.FLAG_WARP | ref.FLAG_FLIP_COLS | ref.FLAG_FLIP_ROWS, 0)


def run(ctx, images, hw, affine, flags, mode, cval, std, expect_error=False, misalign=0, call=None):
    """-> x float32 (B, 3, H, W) from wsc_cls_train_batch on guarded buffers (misalign: bytes x_dev is moved off the 16-byte grid);
    expect_error: the error text of a WSC_ERR_INVALID that left the output alone.  call(src_ptr, x_ptr): another way to call."""
    B, (H, W) = len(images), hw
    img, off = _pack(images)
    src, out = Guarded(ctx, img.size, img), Guarded(ctx, B * 3 * H * W * 4 + misalign)
    try:
        if call is None:
            call = lambda s, x: _lib.cls_train_batch(ctx, s, [i.shape[:2] for i in images], off[:-1], hw, np.asarray(affine, np.float64),  # noqa: E731
                                                     np.asarray(flags, np.int32), mode, cval, std[0], std[1], std[2], x)
        if expect_error:
            with pytest.raises(_lib.WscError) as ei:
                call(src.ptr, out.ptr + misalign)
            assert ei.value.status == _lib.WSC_ERR_INVALID
            ctx.sync()
            assert (out.payload("x") == SENTINEL).all(), "a refused call wrote to x"
            return str(ei.value)
        call(src.ptr, out.ptr + misalign)
        raw = out.payload("x")
        assert (raw[:misalign] == SENTINEL).all()
        assert np.array_equal(src.payload("packed images"), img)
        return raw[misalign:].copy().view(np.float32).reshape(B, 3, H, W)
    finally:
        src.free()
        out.free()


def same_bits(got, want, what):
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert got.shape == want.shape and not diff.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist(), got[diff][0], want[diff][0])


def check(ctx, images, hw, affine, flags, mode, cval, std, what, **kw):
    got = run(ctx, images, hw, affine, flags, mode, cval, std, **kw)
    same_bits(got, ref.batch(images, hw, affine, flags, mode, cval, *std), what)
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", ref.TARGETS)
def test_fixed_transforms(ctx, hw, mode):
    """B = 5 with mixed flags in one batch -- warp on and off, each flip, both -- over the five sources, and B = 1"""
    srcs = ref.sources_for(hw)
    for n, (name, a) in enumerate(ref.named_affines(*hw).items()):
        images = [ref.image(200 + n + k, srcs[(k + n) % 5]) for k in range(5)]
        flags = [MIXED_FLAGS[(k + n) % 5] for k in range(5)]
        std, cval = ref.STANDARDISE[DATASETS[n % 3]], ref.CVALS[n % 2]
        check(ctx, images, hw, [a] * 5, flags, mode, cval, std, (name, "B=5"))
        check(ctx, images[n % 5:n % 5 + 1], hw, [a], [ref.FLAG_WARP | ((n % 4) << 1)], mode, cval, std, (name, "B=1"))


@pytest.mark.parametrize("dataset", DATASETS)
def test_voc_draws_and_the_three_standardisations(ctx, dataset):
    for seed in range(6):
        hw = ref.TARGETS[1:][seed % 3]
        srcs = ref.sources_for(hw)
        affine, flags = ref.voc_draws(seed, hw[0], hw[1], 5)
        images = [ref.image(300 + seed + k, srcs[(k + seed) % 5]) for k in range(5)]
        check(ctx, images, hw, affine, flags, MODES[seed % 3], ref.CVALS[seed % 2], ref.STANDARDISE[dataset], seed)


def test_flagged_identity_equals_the_unflagged_sample_and_calls_repeat(ctx):
    hw = (17, 33)
    images = [ref.image(11 + k, s) for k, s in enumerate(ref.sources_for(hw))]
    std = ref.STANDARDISE["VOC2012"]
    for mode in MODES:
        flipped = [0, ref.FLAG_FLIP_COLS, ref.FLAG_FLIP_ROWS, ref.FLAG_FLIP_COLS | ref.FLAG_FLIP_ROWS, 0]
        plain = run(ctx, images, hw, [ref.IDENTITY] * 5, flipped, mode, 37.5, std)
        warped = run(ctx, images, hw, [ref.IDENTITY] * 5, [f | ref.FLAG_WARP for f in flipped], mode, 37.5, std)
        same_bits(warped, plain, mode)
    affine, flags = ref.voc_draws(3, hw[0], hw[1], 5)
    a = run(ctx, images, hw, affine, flags, "reflect", 0.0, std)
    b = run(ctx, images, hw, affine, flags, "reflect", 0.0, std)
    same_bits(a, b, "two calls")


def test_output_off_the_16_byte_grid_takes_the_scalar_path(ctx):
    hw = (17, 33)  # 5 * 3 * 17 * 33 floats: 8415, three of them behind the last whole 16-byte word
    images = [ref.image(21 + k, s) for k, s in enumerate(ref.sources_for(hw))]
    affine, flags = ref.voc_draws(4, hw[0], hw[1], 5)
    for misalign in (0, 4, 8, 12):
        check(ctx, images, hw, affine, flags, "reflect", 0.0, ref.STANDARDISE["ADP"], misalign, misalign=misalign)


def test_full_size_batch(ctx):
    """321 x 321 at B = 2 from 500 x 375 (and 375 x 500) sources: the one full-size case, for the width of the indices"""
    hw = (321, 321)
    images = [ref.image(31, (375, 500)), ref.image(32, (500, 375))]
    affine, flags = ref.voc_draws(5, 321, 321, 2)
    check(ctx, images, hw, affine, flags, "reflect", 0.0, ref.STANDARDISE["VOC2012"], "321")


def test_refusals_launch_nothing(ctx):
    hw = (8, 8)
    images = [ref.image(41, (16, 16)), ref.image(42, (5, 23)), ref.image(43, (8, 8))]
    std = ref.STANDARDISE["VOC2012"]
    good = np.array([ref.IDENTITY] * 3, np.float64)
    flags = [ref.FLAG_WARP] * 3
    for what, k, value in (("nan matrix", 1, np.nan), ("inf matrix", 2, np.inf), ("nan offset", 4, np.nan), ("inf offset", 5, -np.inf),
                           ("far row", 4, 2.0 ** 20 + 8.5), ("far column", 5, -(2.0 ** 20) - 1.5), ("far through the matrix", 3, 2.0 ** 18)):
        bad = good.copy()
        bad[1, k] = value
        msg = run(ctx, images, hw, bad, flags, "reflect", 0.0, std, expect_error=True)
        assert "sample 1" in msg, (what, msg)
        # ... and the same numbers are not looked at where the sample is not warped
        check(ctx, images, hw, np.nan_to_num(bad, nan=0.0, posinf=0.0, neginf=0.0), [ref.FLAG_WARP, 0, ref.FLAG_WARP], "reflect", 0.0, std, what)
    just_inside = good.copy()
    just_inside[1, 5] = 2.0 ** 20  # column 7 maps to 2^20 + 7 = n - 1 + 2^20: the last accepted value
    check(ctx, images, hw, just_inside, flags, "reflect", 0.0, std, "2^20")
    assert "sample 2" in run(ctx, images, hw, good, [1, 1, 8], "reflect", 0.0, std, expect_error=True)
    for bad_std in ((std[0], 0.0, std[2]), (std[0], np.nan, std[2]), (std[0], std[1], np.inf), ((104.0, np.nan, 123.0), std[1], std[2])):
        run(ctx, images, hw, good, flags, "reflect", 0.0, bad_std, expect_error=True)
    run(ctx, images, hw, good, flags, "reflect", np.inf, std, expect_error=True)
    for mode in (3, -1):  # 3 would be scipy's 'wrap'
        assert "fill_mode" in run(ctx, images, hw, good, flags, mode, 0.0, std, expect_error=True)
    with pytest.raises(ValueError):
        _lib.cls_train_batch(ctx, 4096, [(8, 8)], [0], hw, good[:1], [1], "wrap", 0.0, std[0], std[1], std[2], 8192)

    # B, H, W: through the C entry itself
    sizes, offs = np.array([i.shape[:2] for i in images], np.int32), np.array([0, 768, 768 + 345], np.int64)
    fl, sub = np.array(flags, np.int32), np.array(std[0], np.float32)

    def raw(B, H, W):
        def call(s, x):
            _lib.check(ctx._lib.wsc_cls_train_batch(ctx.h, s, B, sizes.ctypes.data, offs.ctypes.data, H, W, good.ctypes.data, fl.ctypes.data, 1,
                                                    ctypes.c_float(0.0), sub.ctypes.data, ctypes.c_float(1.0), ctypes.c_float(1.0), x))
        return call

    for B, H, W in ((0, 8, 8), (65536, 8, 8), (-1, 8, 8), (3, 0, 8), (3, 8, 0), (3, -1, 8)):
        run(ctx, images, hw, good, flags, "reflect", 0.0, std, expect_error=True, call=raw(B, H, W))
    check(ctx, images, hw, good, flags, "reflect", 0.0, (std[0], 1.0, 1.0), "raw", call=raw(3, 8, 8))
