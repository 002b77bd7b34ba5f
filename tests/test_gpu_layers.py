"""GPU: the small kernels between the convolutions, one layer at a time against the float64 references of tests/layer_ref.py --
the GroupNorm of the IRNet heads (csrc/irn_kernels.hip: two statistics kernels, four apply kernels), nn.MaxPool2d
(csrc/pool.hip: four kernels, shared with the TF / Keras pools), the classifier branch (gap + linear + sigmoid), flip-add and the IRNet edge finish.  The
entries (wsc_group_norm_nhwc, wsc_maxpool_nhwc, wsc_gap_linear_sigmoid, wsc_cam_flip_add, wsc_irn_edge_finish) stage float32 into
the activation planes of a precision and run the production launchers unchanged.

Bars.  A maximum, a ReLU and a copy add no rounding: they are held to equality on the values the planes hold
(layer_ref.as_precision).  Everything else has a bound DERIVED from its arithmetic, stated where it is used; each test prints
its worst err / tol.  Inputs have both signs everywhere (after a ReLU a zero-padded pool or a dropped sign passes unnoticed)."""
import numpy as np
import pytest

from tests import layer_ref as lr
from wsscam import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # the unit round-off of fp32
H16 = (_lib.PREC_BF16, _lib.PREC_BF16X3, _lib.PREC_F16, _lib.PREC_F16X3)


def _prec_id(p):
    return lr.PREC_NAME[p]


# ---- nn.MaxPool2d ---------------------------------------------------------------------------------------------------------------
def _run_pool(ctx, x, entry, *args):
    N, H, W, C = x.shape
    x_dev = ctx.to_device(x)
    try:
        y_dev, shp = entry(ctx, x_dev, N, H, W, C, *args)
        y = ctx.to_host(y_dev, shp, np.float32)
        y_dev.free()
        return y
    finally:
        x_dev.free()


def _maxpool(ctx, x, k, stride, pad, prec):
    return _run_pool(ctx, x, _lib.maxpool_nhwc, k, stride, pad, prec)


def _assert_pool_exact(ctx, x, k, stride, pad, prec):
    v = lr.as_precision(x, prec)
    want = lr.max_pool(v, k, stride, pad)
    y = _maxpool(ctx, x, k, stride, pad, prec)
    assert y.shape == want.shape, (lr.PREC_NAME[prec], y.shape, want.shape)
    bad = y.astype(np.float64) != want
    assert not bad.any(), (lr.PREC_NAME[prec], int(bad.sum()), np.argwhere(bad)[:4].tolist(), y[bad][:4], want[bad][:4])
    return want


POOL_CASES = [(3, 2, 1, 7, 9), (3, 2, 1, 8, 8), (3, 2, 1, 1, 1), (2, 2, 0, 2, 2), (2, 2, 0, 5, 4), (2, 2, 0, 7, 9), (2, 2, 0, 8, 8)]


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("geom", POOL_CASES, ids=lambda g: "k%ds%dp%d-%dx%d" % g)
def test_maxpool_exact(ctx, geom, C):
    """Every precision (bf16 / bf16x3: pool_h16_kernel; f16: maxpool_f16_kernel; f16x3: maxpool_f16x2_kernel; f32:
    pool_f32_kernel) returns exactly the maximum of the values its planes hold: odd sizes whose last row / column is dropped
    (2 x 2 / 2) or is padding (3 x 3 / 2 pad 1), a 1 x 1 map that is all border, signed values."""
    k, stride, pad, H, W = geom
    rng = np.random.default_rng(H * 1000 + W * 10 + k + C)
    x = (rng.normal(0, 3, (3, H, W, C)) - 1.0).astype(np.float32)
    for prec in lr.ALL_PRECISIONS:
        want = _assert_pool_exact(ctx, x, k, stride, pad, prec)
        assert (want < 0).any() and (want > 0).any()


@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
def test_maxpool_all_negative(ctx, prec):
    """Every value negative: a pool that counted a padding tap as 0 (or started from 0) is wrong at every border window."""
    rng = np.random.default_rng(7)
    x = (-np.abs(rng.normal(0, 3, (3, 7, 9, 72))) - 2.0 ** -6).astype(np.float32)
    want = _assert_pool_exact(ctx, x, 3, 2, 1, prec)
    assert (want < 0).all()
    _assert_pool_exact(ctx, x[:, :5, :4, :8].copy(), 2, 2, 0, prec)


@pytest.mark.parametrize("prec", lr.TWO_PLANE, ids=_prec_id)
def test_maxpool_lo_plane_decides(ctx, prec):
    """Two-plane modes: within a channel every value has the SAME hi plane (of either sign) and the lo plane alone decides the
    maximum -- a pool on the hi plane, or one that re-split a negative maximum wrongly, returns another value."""
    rng = np.random.default_rng(11)
    N, H, W, C = 3, 7, 9, 8
    base = np.array([1.5, -2.25, 0.375, -0.75, 3.0, -1.0, 0.5, -6.5], np.float32)  # 16-bit values whose neighbours are > 6 * 2^-15 away
    j = rng.integers(-3, 4, (N, H, W, C)).astype(np.float32)
    x = base + j * np.float32(2.0 ** -15)
    hi, lo = lr.planes(x, prec)
    assert np.array_equal(hi, np.broadcast_to(base, x.shape)) and np.array_equal(lo, j * np.float32(2.0 ** -15))
    assert np.array_equal(lr.as_precision(x, prec), x)
    for k, stride, pad in ((3, 2, 1), (2, 2, 0)):
        want = _assert_pool_exact(ctx, x, k, stride, pad, prec)
        assert len(np.unique(want - base)) > 3  # (the maxima differ in their lo planes only)


@pytest.mark.parametrize("prec", [_lib.PREC_F16, _lib.PREC_F16X3], ids=_prec_id)
def test_maxpool_many_rows_takes_generic_kernel(ctx, prec):
    """N * Ho = 65536 > 65535: the IEEE-half modes leave their one-block-row-per-output-row kernels for pool_h16_kernel with the
    half format (launch_pool's `rows`).  2 x 2 / 2 on 2 x 2 maps: the result is the maximum of each sample's four pixels."""
    rng = np.random.default_rng(13)
    x = (rng.normal(0, 3, (65536, 2, 2, 8)) - 1.0).astype(np.float32)
    want = lr.as_precision(x, prec).reshape(65536, 4, 8).max(1).reshape(65536, 1, 1, 8)
    y = _maxpool(ctx, x, 2, 2, 0, prec)
    assert y.shape == want.shape and np.array_equal(y, want)
    assert (want < 0).any() and (want > 0).any()


# ---- one launcher behind three entries (csrc/pool.hip) --------------------------------------------------------------------------
def _pool_same(ctx, x, avg, stride, prec):
    return _run_pool(ctx, x, _lib.pool_same_nhwc, avg, stride, prec)


def _pool_tf(ctx, x, k, stride, same, prec):
    return _run_pool(ctx, x, _lib.pool_tf_nhwc, k, stride, same, prec)


def test_pool_entries_agree_where_their_rules_coincide(ctx):
    """wsc_maxpool_nhwc, wsc_pool_same_nhwc and wsc_pool_tf_nhwc are one launcher under three rules.  On an odd size torch's
    3 / 2 / pad 1 and TF SAME 3 / 2 are the same windows (one row / column of padding on either side), and without padding
    torch's 2 / 2 / 0 is TF VALID 2 / 2: identical arrays in every precision.  On an even size TF SAME pads AFTER (0 / 1) where
    torch pads before and drops nothing: the two must DIFFER in the last output row and column -- three entries that ignored
    their rule would agree -- while each still equals its own float64 reference."""
    from tests import keras_arch_ref as kref

    rng = np.random.default_rng(29)
    for prec in lr.ALL_PRECISIONS:
        for C in (8, 72):
            x = (rng.normal(0, 3, (3, 7, 9, C)) - 1.0).astype(np.float32)
            assert (x < 0).any() and (x > 0).any()
            torch_y = _maxpool(ctx, x, 3, 2, 1, prec)
            assert torch_y.shape == (3, 4, 5, C)
            assert np.array_equal(torch_y, _pool_same(ctx, x, False, 2, prec)), (lr.PREC_NAME[prec], C)
            assert np.array_equal(torch_y, _pool_tf(ctx, x, 3, 2, 1, prec)), (lr.PREC_NAME[prec], C)
        x = (rng.normal(0, 3, (3, 5, 4, 8)) - 1.0).astype(np.float32)
        assert np.array_equal(_maxpool(ctx, x, 2, 2, 0, prec), _pool_tf(ctx, x, 2, 2, 0, prec)), lr.PREC_NAME[prec]
        x = (rng.normal(0, 3, (3, 8, 8, 8)) - 1.0).astype(np.float32)
        v = lr.as_precision(x, prec)
        torch_y, same_y, tf_y = _maxpool(ctx, x, 3, 2, 1, prec), _pool_same(ctx, x, False, 2, prec), _pool_tf(ctx, x, 3, 2, 1, prec)
        assert np.array_equal(same_y, tf_y)
        assert not np.array_equal(torch_y[:, -1], tf_y[:, -1]) and not np.array_equal(torch_y[:, :, -1], tf_y[:, :, -1]), lr.PREC_NAME[prec]
        assert np.array_equal(torch_y.astype(np.float64), lr.max_pool(v, 3, 2, 1)), lr.PREC_NAME[prec]
        assert np.array_equal(tf_y.astype(np.float64), kref.tf_max_pool(v, 3, 2, True)), lr.PREC_NAME[prec]


@pytest.mark.parametrize("prec", [_lib.PREC_F16, _lib.PREC_F16X3], ids=_prec_id)
def test_pool_tf_many_rows_takes_generic_kernel(ctx, prec):
    """The twin of test_maxpool_many_rows_takes_generic_kernel under the TF VALID rule: N * Ho = 65536 > 65535, so pool_h16_kernel
    with the half format runs in place of a row kernel.  2 x 2 / 2 on 2 x 2 maps: the maximum of each sample's four pixels."""
    rng = np.random.default_rng(31)
    x = (rng.normal(0, 3, (65536, 2, 2, 8)) - 1.0).astype(np.float32)
    want = lr.as_precision(x, prec).reshape(65536, 4, 8).max(1).reshape(65536, 1, 1, 8)
    y = _pool_tf(ctx, x, 2, 2, 0, prec)
    assert y.shape == want.shape and np.array_equal(y, want)
    assert (want < 0).any() and (want > 0).any()


@pytest.mark.parametrize("prec", [_lib.PREC_F16, _lib.PREC_F16X3], ids=_prec_id)
def test_pool_tf_asymmetric_padding_on_row_kernel(ctx, prec):
    """TF SAME 3 / 2 on an even 8 x 6 map, the IEEE-half row kernels (maxpool_f16_kernel / maxpool_f16x2_kernel): no padding
    before (pad_t = pad_l = 0), one row / column after.  Every value negative: a kernel that still applied a symmetric pad reads
    other windows, one that let the padding win returns 0 -- both show at the last row / column."""
    from tests import keras_arch_ref as kref

    rng = np.random.default_rng(37)
    x = (-np.abs(rng.normal(0, 3, (3, 8, 6, 8))) - 2.0 ** -6).astype(np.float32)
    want = kref.tf_max_pool(lr.as_precision(x, prec), 3, 2, True)
    y = _pool_tf(ctx, x, 3, 2, 1, prec)
    assert y.shape == want.shape == (3, 4, 3, 8)
    assert np.array_equal(y.astype(np.float64), want), np.argwhere(y != want)[:4].tolist()
    assert (want < 0).all()


# ---- GroupNorm head -------------------------------------------------------------------------------------------------------------
def _gn_data(rng, N, H, W, C, G, kind):
    Cg = C // G
    if kind == "offset":  # mean 100, standard deviation 0.05: pins E[x^2] - mean^2 against the two-pass reference
        x = (100.0 + 0.05 * rng.normal(0, 1, (N, H, W, C))).astype(np.float32)
    else:
        x = (rng.normal(0, 1, (N, H, W, C)) * rng.uniform(0.5, 3.0, C) + rng.normal(0, 1.5, C)).astype(np.float32)
        assert (x < 0).any() and (x > 0).any()
    if kind == "constant":  # group 1 of sample 0 has variance 0
        x[0, :, :, Cg:2 * Cg] = np.float32(1.7)
    gamma = rng.normal(0, 1, C).astype(np.float32)
    gamma[0], gamma[1], gamma[2] = -abs(gamma[0]) - 0.1, 0.0, abs(gamma[2]) + 0.1
    if kind == "constant":
        gamma[Cg] = 1.25
    beta = (rng.normal(0, 1, C) + np.where(rng.random(C) < 0.5, -0.5, 0.5)).astype(np.float32)
    return x, gamma, beta


def _ramp(Ctot):
    """the sentinel of the concat buffer: one value per channel, far above anything a normalised head writes"""
    return (1000.0 + 37.0 * np.arange(Ctot)).astype(np.float32)


def _gn_run(ctx, x, gamma, beta, G, up, relu, Hd, Wd, Ctot, coff, prec, eps=1e-5):
    N, H, W, C = x.shape
    y0 = np.ascontiguousarray(np.broadcast_to(_ramp(Ctot), (N, Hd, Wd, Ctot)))
    x_dev, y_dev = ctx.to_device(x), ctx.to_device(y0)
    try:
        _lib.group_norm_nhwc(ctx, x_dev, N, H, W, C, gamma, beta, G, eps, up, relu, Hd, Wd, Ctot, coff, prec, y_dev)
        return ctx.to_host(y_dev, (N, Hd, Wd, Ctot), np.float32)
    finally:
        x_dev.free()
        y_dev.free()


def _gn_check(ctx, x, gamma, beta, G, up, relu, Hd, Wd, Ctot, coff, prec, eps=1e-5):
    """-> worst err / tol of the slice.  The bound, per element of channel c in group g of sample n:
        tol = 16 * 2^-24 * (|gamma_c| * rstd * (max|x| over the group + |mean|) + |beta_c|) + q * |ref| + floor
    First term: the fp32 chain.  mean and rstd are each stored as fp32 (the sums behind them are double), then come the
    subtraction, two products, the add and three lerp operations -- at most 10 roundings, each relative to an intermediate no
    larger than |gamma| rstd (max|x| + |mean|) + |beta| (the lerp is a convex combination of the group's values); 16 leaves
    margin for the order the operations are fused in.  q: the half-ulp of the value the planes hold (bf16 2^-8, f16 2^-11, bf16x3
    2^-16, f16x3 2^-22, f32 0); floor = 2^-25 in the IEEE-half modes (subnormal spacing 2^-24).  Nothing here is measured."""
    N, H, W, C = x.shape
    Cg = C // G
    ramp = _ramp(Ctot)
    y = _gn_run(ctx, x, gamma, beta, G, up, relu, Hd, Wd, Ctot, coff, prec, eps)
    # the sentinel property: the other heads' channels come back as the planes hold them, the slice holds no sentinel
    keep = np.ones(Ctot, bool)
    keep[coff:coff + C] = False
    want_keep = np.broadcast_to(lr.as_precision(ramp, prec)[keep], (N, Hd, Wd, int(keep.sum())))
    assert np.array_equal(y[..., keep], want_keep), "channels outside [%d, %d) changed" % (coff, coff + C)
    sl = y[..., coff:coff + C]
    assert (np.abs(sl) < 500.0).all(), "a sentinel (or worse) inside the slice"
    ref = lr.group_norm_head(x, gamma, beta, G, eps, up, relu, Hd, Wd, np.zeros((N, Hd, Wd, Ctot)), coff)[..., coff:coff + C]
    mean, rstd, amax = lr.group_stats(x, G, eps)
    scale = np.repeat(rstd * (amax + np.abs(mean)), Cg, axis=1)  # (N, C)
    chain = 16 * U * (np.abs(gamma.astype(np.float64)) * scale + np.abs(beta.astype(np.float64)))  # (N, C)
    tol = chain[:, None, None, :] + lr.HALF_ULP[prec] * np.abs(ref) + lr.ABS_FLOOR[prec]
    err = np.abs(sl.astype(np.float64) - ref)
    worst = float((err / tol).max())
    i = np.unravel_index(np.argmax(err / tol), err.shape)
    assert worst <= 1.0, "err / tol = %.3f at %s: got %r, reference %r, tol %.3e" % (worst, i, sl[i], ref[i], tol[i])
    if relu:
        assert (sl >= 0).all()
    return worst


# statistics kernel by C / G (launch_group_norm_stats): (C / G) % 4 == 0 -> gn_partial4_kernel, else gn_partial_kernel
GN_STATS_SHAPES = [pytest.param(6, 3, 10, 3, id="C6G3-gn_partial_kernel+gn_apply_kernel"),
                   pytest.param(12, 3, 16, 4, id="C12G3-gn_partial4_kernel+gn_apply_kernel"),
                   pytest.param(32, 4, 192, 64, id="C32G4of192at64-gn_partial4_kernel+gn_apply8_kernel")]
GN_MAPS = [(1, 1), (3, 5), (33, 31), (32, 32), (25, 41), (47, 47)]  # 1, 15, 1023, 1024, 1025 pixels and three chunks of GN_CHUNK


@pytest.mark.parametrize("hw", GN_MAPS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C,G,Ctot,coff", GN_STATS_SHAPES)
def test_group_norm_statistics_and_chunks(ctx, C, G, Ctot, coff, hw):
    """Both statistics kernels at every GN_CHUNK = 1024 boundary, two samples and more than one group (a wrong sample, group or
    chunk stride moves the statistics), no upsampling: the error is the statistics' and the affine map's."""
    H, W = hw
    rng = np.random.default_rng(C * 10000 + H * 100 + W)
    worst = 0.0
    for kind, relu in (("plain", 0), ("offset", 1), ("constant", 0)):
        x, gamma, beta = _gn_data(rng, 2, H, W, C, G, kind)
        for prec in (_lib.PREC_F16X3, _lib.PREC_BF16):
            worst = max(worst, _gn_check(ctx, x, gamma, beta, G, 1, relu, H, W, Ctot, coff, prec))
    print("worst err/tol %.3f" % worst)


# apply kernel by the slice (launch_group_norm_apply): fp32 planes -> gn_apply_f32_kernel; C, Ctot, coff all multiples of 8 ->
# gn_apply8_kernel<false> (up = 1) / <true> (up > 1); else gn_apply_kernel
GN_APPLY_SHAPES = [pytest.param(12, 3, 12, 0, H16, id="C12-gn_apply_kernel"),
                   pytest.param(16, 2, 24, 4, H16, id="C16of24at4-gn_apply_kernel"),
                   pytest.param(16, 2, 24, 8, H16, id="C16of24at8-gn_apply8_kernel"),
                   pytest.param(32, 4, 192, 64, H16, id="C32of192at64-gn_apply8_kernel"),
                   pytest.param(12, 3, 16, 4, (_lib.PREC_F32,), id="C12of16at4-gn_apply_f32_kernel"),
                   pytest.param(32, 4, 192, 64, (_lib.PREC_F32,), id="C32of192at64-gn_apply_f32_kernel")]
# (H, W, up, Hd, Wd): the crop strictly inside H up x W up and the full map (its clamped last row and column) for every factor
GN_UPS = [(3, 5, 1, 2, 4), (3, 5, 1, 3, 5), (3, 5, 2, 5, 9), (3, 5, 2, 6, 10), (5, 7, 4, 17, 26), (5, 7, 4, 20, 28), (1, 1, 4, 4, 3),
          (2, 1, 2, 4, 2)]


@pytest.mark.parametrize("geom", GN_UPS, ids=lambda g: "%dx%dup%dto%dx%d" % g)
@pytest.mark.parametrize("C,G,Ctot,coff,precs", GN_APPLY_SHAPES)
def test_group_norm_apply_upsample_crop(ctx, C, G, Ctot, coff, precs, geom):
    """Every apply kernel with the upsampling factors of the nets (1 / up is exact: the source coordinates are), a crop, the
    clamped border taps, with and without ReLU, into a slice of a wider concat buffer."""
    H, W, up, Hd, Wd = geom
    rng = np.random.default_rng(C * 1000 + coff * 100 + H * 10 + up)
    x, gamma, beta = _gn_data(rng, 2, H, W, C, G, "plain")
    worst = 0.0
    for prec in precs:
        for relu in (0, 1):
            worst = max(worst, _gn_check(ctx, x, gamma, beta, G, up, relu, Hd, Wd, Ctot, coff, prec))
    print("worst err/tol %.3f" % worst)


@pytest.mark.parametrize("prec", lr.ALL_PRECISIONS, ids=_prec_id)
def test_group_norm_offset_and_constant_upsampled(ctx, prec):
    """The two hard inputs through the upsampling kernels of every precision: a large common offset, and a constant group
    (variance 0, rstd = eps^-1/2: the result is beta up to the tolerance)."""
    rng = np.random.default_rng(17)
    worst = 0.0
    for kind in ("offset", "constant"):
        x, gamma, beta = _gn_data(rng, 2, 6, 5, 16, 2, kind)
        for coff in (4, 8):
            worst = max(worst, _gn_check(ctx, x, gamma, beta, 2, 2, 0, 11, 10, 24, coff, prec))
    print("worst err/tol %.3f" % worst)


@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("prec", [_lib.PREC_F16X3, _lib.PREC_BF16], ids=_prec_id)
def test_group_norm_scalar_and_vector_kernels_same_bits(ctx, prec, up):
    """irn_kernels.hip promises that every element of gn_apply8_kernel goes through the expressions of gn_apply_kernel (same
    bits).  The same head into channels [4, 20) (scalar kernel) and [8, 24) (vector kernel) of a 24-channel buffer."""
    rng = np.random.default_rng(19 + up)
    H, W = 7, 9
    Hd, Wd = H * up, W * up - (1 if up > 1 else 0)
    x, gamma, beta = _gn_data(rng, 2, H, W, 16, 2, "plain")
    for relu in (0, 1):
        a = _gn_run(ctx, x, gamma, beta, 2, up, relu, Hd, Wd, 24, 4, prec)[..., 4:20]
        b = _gn_run(ctx, x, gamma, beta, 2, up, relu, Hd, Wd, 24, 8, prec)[..., 8:24]
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert not diff.any(), (int(diff.sum()), a[diff][:4], b[diff][:4])
        assert len(np.unique(a)) > 50  # (not a buffer of constants)


# ---- classifier branch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [64, 72, 512])
@pytest.mark.parametrize("npix", [1, 5, 25, 63, 1681])
def test_gap_linear_sigmoid(ctx, npix, F):
    """gap_kernel / gap_f32_kernel + linear_sigmoid_kernel against float64 on the values the planes hold.

    The pooled value.  16 waves sum contiguous runs of ceil(npix / 16) positions in fp32 (waves past the end have empty runs,
    npix < 128 leaves every run shorter than the unroll of 8), wave 0 adds the 16 partial sums, then one division: a chain of at
    most ceil(npix / 16) + 16 roundings, each relative to a partial sum no larger than sum|v|.  Recursive summation:
        |gap - exact| <= (ceil(npix / 16) + 16) * 2^-24 * mean|v|        (0 for the global max: a maximum is exact)
    The dot product.  A lane multiplies and adds its F / 64 terms, six shuffle steps add the lanes: F / 64 + 7 roundings on
    partial sums bounded by sum|W gap|, on top of the pooled error carried through |W|:
        |z - exact| <= sum_f |W_cf| bound_f + (F / 64 + 7) * 2^-24 * sum_f |W_cf gap_f|
    The sigmoid has slope <= 1/4; expf, the add and the division are within 4 * 2^-24 of the exact sigmoid (values <= 1):
        tol = |z - exact| / 4 + 4 * 2^-24
    sample_stride = 2 reads samples 0, 2, ...; the odd ones hold a large constant, so a wrong stride cannot pass."""
    rng = np.random.default_rng(npix * 1000 + F)
    B = 2
    feat = (rng.normal(0, 1, (2 * B, npix, F)) * rng.uniform(0.2, 2.0, F) + rng.normal(0, 0.5, F)).astype(np.float32)
    feat[1::2] = 1.0e4
    assert (feat[0::2] < 0).any() and (feat[0::2] > 0).any()
    packed = np.ascontiguousarray(feat[0::2])  # the same samples back to back, for sample_stride = 1
    negative = (-np.abs(packed) - 0.125).astype(np.float32)
    w20 = rng.normal(0, 1, (20, F))
    b20 = rng.normal(0, 0.5, 20).astype(np.float32)
    # (features, C, bias, sample_stride, global max)
    combos = [(feat, 20, True, 2, False), (packed, 1, False, 1, False), (packed, 20, False, 1, True), (feat, 1, True, 2, True),
              (negative, 20, True, 1, True)]
    worst = 0.0
    for prec in (_lib.PREC_F16X3, _lib.PREC_BF16, _lib.PREC_F32):
        for fe, C, with_bias, stride, use_max in combos:
            # (the weights scaled so that the logits stay within +-3 and the sigmoid away from saturation, whatever the pool)
            z0 = lr.gap(fe, use_max, stride) @ w20[:C].T
            w, bias = (w20[:C] * (3.0 / np.abs(z0).max())).astype(np.float32), (b20[:C] if with_bias else None)
            f_dev = ctx.to_device(fe)
            try:
                s_dev, shp = _lib.gap_linear_sigmoid(ctx, f_dev, B, -npix if use_max else npix, F, w, bias, stride, prec)
                score = ctx.to_host(s_dev, shp, np.float32)
                s_dev.free()
            finally:
                f_dev.free()
            v = lr.as_precision(fe, prec)
            ref, g = lr.gap_linear_sigmoid(v, w, bias, use_max, stride)
            if use_max and fe is negative:
                assert (g < 0).all()
            gb = np.zeros_like(g) if use_max else (-(-npix // 16) + 16) * U * np.abs(v.astype(np.float64)[::stride]).mean(1)  # (B, F)
            aw = np.abs(w.astype(np.float64))
            zb = gb @ aw.T + (F / 64 + 7) * U * (np.abs(g) @ aw.T)
            tol = zb / 4 + 4 * U
            err = np.abs(score.astype(np.float64) - ref)
            r = float((err / tol).max())
            assert r <= 1.0, (lr.PREC_NAME[prec], C, with_bias, stride, use_max, r, float(err.max()))
            assert ref.min() > 1e-3 and ref.max() < 1 - 1e-3  # (the sigmoid is not saturated: the bound is not vacuous)
            worst = max(worst, r)
    print("worst err/tol %.3f" % worst)


# ---- flip-add and the IRNet edge finish -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (4, 6)], ids=lambda s: "%dx%d" % s)
def test_cam_flip_add_exact(ctx, hw):
    """cam = relu(a) + relu(flip(b)): one rounding of an exact sum of two fp32 values on both sides -> equality.  C = 5 of
    Cs = 8 channels; the padding channels hold a sentinel that must not reach the output."""
    h, w = hw
    B, C, Cs = 2, 5, 8
    rng = np.random.default_rng(h * 10 + w)
    head = rng.normal(0, 2, (2 * B, h, w, Cs)).astype(np.float32)
    head[..., C:] = 7.0e5
    assert (head[..., :C] < 0).any() and (head[..., :C] > 0).any()
    h_dev = ctx.to_device(head)
    try:
        c_dev, shp = _lib.cam_flip_add(ctx, h_dev, B, h, w, C, Cs)
        cam = ctx.to_host(c_dev, shp, np.float32)
        c_dev.free()
    finally:
        h_dev.free()
    want = lr.flip_add(head, C)
    assert want.dtype == np.float32 and cam.shape == want.shape == (B, C, h, w)
    assert np.array_equal(cam, want), np.abs(cam - want).max()


# (He, We, Hd, Wd, fh, fw)
EDGE_CASES = [pytest.param(6, 8, 6, 8, 4, 5, id="crop-fh<He-fw<We-odd-fw"), pytest.param(8, 10, 4, 5, 4, 5, id="m7-He!=Hd"),
              pytest.param(3, 4, 3, 4, 3, 4, id="full-even-fw"), pytest.param(1, 3, 2, 2, 1, 1, id="1x1")]


@pytest.mark.parametrize("He,We,Hd,Wd,fh,fw", EDGE_CASES)
def test_irn_edge_finish(ctx, He, We, Hd, Wd, fh, fw):
    """The crop precedes the flip: column fw - 1 - x of the CROPPED map is read, not We - 1 - x.  dp = d - mean shift is one fp32
    subtraction on both sides (equality).  edge: e / 2 is exact, the sum one rounding (|z| 2^-24, through a slope <= 1/4), expf,
    the add and the division are within a few 2^-24 of the exact sigmoid of values <= 1: bound 4 * 2^-24."""
    B = 2
    rng = np.random.default_rng(He * 100 + We * 10 + fw)
    e = rng.normal(0, 2, (2 * B, He, We)).astype(np.float32)
    d = rng.normal(0, 3, (2 * B, Hd, Wd, 2)).astype(np.float32)
    ms = (np.float32(0.375), np.float32(-1.625))
    e_dev, d_dev = ctx.to_device(e), ctx.to_device(d)
    try:
        edge_dev, dp_dev = _lib.irn_edge_finish(ctx, e_dev, He, We, d_dev, Hd, Wd, B, fh, fw, ms[0], ms[1])
        edge, dp = ctx.to_host(edge_dev, (B, fh, fw), np.float32), ctx.to_host(dp_dev, (B, 2, fh, fw), np.float32)
        edge_dev.free()
        dp_dev.free()
    finally:
        e_dev.free()
        d_dev.free()
    want_edge, want_dp = lr.edge_finish(e, d, fh, fw, ms)
    assert want_dp.dtype == np.float32 and np.array_equal(dp, want_dp)
    r = float(np.abs(edge.astype(np.float64) - want_edge).max() / (4 * U))
    print("worst err/tol %.3f" % r)
    assert r <= 1.0


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_entry_argument_checks(ctx):
    """A bad argument is WSC_ERR_INVALID before anything is launched; the context works afterwards."""
    x = np.random.default_rng(23).normal(0, 1, (2, 4, 4, 8)).astype(np.float32)
    g, b = np.ones(8, np.float32), np.zeros(8, np.float32)
    x_dev, y_dev = ctx.to_device(x), ctx.to_device(np.zeros((2, 8, 8, 8), np.float32))
    P = _lib.PREC_F16X3

    def gn(xd=x_dev, yd=y_dev, gamma=g, beta=b, C=8, G=2, up=1, Hd=4, Wd=4, Ctot=8, coff=0, prec=P):
        return lambda: _lib.group_norm_nhwc(ctx, xd, 2, 4, 4, C, gamma, beta, G, 1e-5, up, 0, Hd, Wd, Ctot, coff, prec, yd)

    def pool(xd=x_dev, yd=y_dev, C=8, k=3, stride=2, pad=1, prec=P):
        return lambda: _lib.maxpool_nhwc(ctx, xd, 2, 4, 4, C, k, stride, pad, prec, yd)

    bad = {"gn null x": gn(xd=None), "gn null y": gn(yd=None), "gn null gamma": gn(gamma=None), "gn null beta": gn(beta=None),
           "gn C % G": gn(G=3), "gn up 3": gn(up=3), "gn crop rows": gn(up=2, Hd=9, Wd=8), "gn crop columns": gn(Hd=4, Wd=5),
           "gn slice past Ctot": gn(coff=4), "gn precision": gn(prec=9), "gn fp32 slice": gn(C=6, G=2, Ctot=8, prec=_lib.PREC_F32),
           "pool null x": pool(xd=None),
           "pool null y": lambda: _lib.check(ctx._lib.wsc_maxpool_nhwc(ctx.h, x_dev.ptr, 2, 4, 4, 8, 3, 2, 1, P, None)), "pool C % 8": pool(C=4), "pool 2 pad > k": pool(k=3, pad=2),
           "pool precision": pool(prec=-1),
           "gap null feat": lambda: _lib.gap_linear_sigmoid(ctx, None, 1, 16, 8, np.ones((2, 8), np.float32), None, 1, P, y_dev),
           "gap no positions": lambda: _lib.gap_linear_sigmoid(ctx, x_dev, 1, 0, 8, np.ones((2, 8), np.float32), None, 1, P, y_dev),
           "gap stride 3": lambda: _lib.gap_linear_sigmoid(ctx, x_dev, 1, 4, 8, np.ones((2, 8), np.float32), None, 3, P, y_dev),
           "flip-add null": lambda: _lib.cam_flip_add(ctx, None, 1, 4, 4, 5, 8, y_dev),
           "flip-add C > Cs": lambda: _lib.cam_flip_add(ctx, x_dev, 1, 4, 4, 9, 8, y_dev),
           "edge null": lambda: _lib.irn_edge_finish(ctx, x_dev, 4, 4, None, 4, 4, 1, 4, 4, 0.0, 0.0, y_dev, y_dev),
           "edge fw > We": lambda: _lib.irn_edge_finish(ctx, x_dev, 4, 4, x_dev, 4, 4, 1, 4, 5, 0.0, 0.0, y_dev, y_dev),
           "edge fh > Hd": lambda: _lib.irn_edge_finish(ctx, x_dev, 4, 4, x_dev, 3, 4, 1, 4, 4, 0.0, 0.0, y_dev, y_dev)}
    try:
        for name, call in bad.items():
            try:
                call()
            except _lib.WscError as e:
                assert e.status == _lib.WSC_ERR_INVALID, (name, str(e))
            else:
                pytest.fail("%s: no error" % name)
        ctx.sync()
        # y_dev was never written, and a valid call works afterwards
        assert not ctx.to_host(y_dev, (2, 8, 8, 8), np.float32).any()
        y, shp = _lib.maxpool_nhwc(ctx, x_dev, 2, 4, 4, 8, 2, 2, 0, _lib.PREC_F32)
        assert np.array_equal(ctx.to_host(y, shp, np.float32), lr.max_pool(x, 2, 2, 0))
        y.free()
        gn(up=2, Hd=8, Wd=8)()
        out = ctx.to_host(y_dev, (2, 8, 8, 8), np.float32)
        ref = lr.group_norm_head(x, g, b, 2, 1e-5, 2, 0, 8, 8, np.zeros((2, 8, 8, 8)), 0)
        assert np.abs(out - ref).max() < 1e-4
    finally:
        x_dev.free()
        y_dev.free()
