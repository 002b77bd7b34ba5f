"""GPU: the kernels that turn maps into LABELS, one entry point at a time against the float64 references of
tests/label_tail_ref.py -- wsc_sem_seg_finish, wsc_cam_sum_scales, wsc_bilinear_resize (csrc/cam_tail.hip),
wsc_label_unary_from_cam, wsc_ir_label_combine (csrc/ir_label.hip), wsc_hsn_voc_background, wsc_hsn_class_mass (csrc/hsn.hip).
The whole-pipeline tests that reach them accept a share of wrong pixels (for the network and the dense CRF in front);
here every pixel counts.

Bars.  A comparison, a table lookup and a float32 sum in a stated order involve no arithmetic of their own: equality.
wsc_sem_seg_finish interpolates in fp32 and returns labels only, so a label is compared wherever the float64 stack's two
largest entries are more than MARGIN = 1e-5 apart (the bound tests/test_gpu_hsn.py states for fp32 bilinear sampling of
O(1) maps); at most 0.1 % of an image's pixels may fall under that margin and no compared pixel may differ.  The element-wise
HSN stage is held to that file's 2e-6.  Each test prints its worst measured error and its excluded share.

Sizes: every launch here caps its grid (256 x B, 64 x n, 2048, 4096 or 8192 blocks of 256 threads) and goes on in a grid-stride
loop; one case of each test is just large enough to enter it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import label_tail_ref as ref
from wsscam import _lib

pytestmark = pytest.mark.gpu

MARGIN = 1e-5      # fp32 bilinear sampling of O(1) maps against float64 (test_gpu_hsn.py)
MAX_EXCLUDED = 1e-3
GUARD = 0xEE       # fills the bytes behind a packed output


# ---- wsc_sem_seg_finish ---------------------------------------------------------------------------------------------------------
SEED = 18
BG_THRES = 0.25  # a float32 number: the device and the oracle compare against the same value
# (K, h, w) -> up -> crop
RAGGED = [((3, 9, 11), (36, 44), (33, 41)),        # crop below the up-size; the global peak lies in the band the crop removes
          ((2, 94, 125), (375, 500), (375, 500)),  # 187 500 pixels > 256 blocks x 256 threads: the grid-stride loop runs ...
          ((1, 1, 1), (5, 7), (5, 7)),             # ... next to an image most of whose blocks hold no pixel
          ((7, 24, 32), (94, 125), (94, 125)),     # more than four maps
          ((2, 5, 6), (20, 24), (20, 24)),         # all zero: NaN maps, the first of them wins
          ((4, 16, 16), (16, 16), (16, 16))]       # identity resize
ZERO_IMAGE = 4


def _keys_for(b, K):
    """K + 1 keys of image b, distinct within and between the images; the 7-map image holds 255."""
    keys = [(37 * b + 11 * j + 1) % 251 for j in range(K + 1)]
    if K == 7:
        keys[-1] = 255
    assert len(set(keys)) == K + 1
    return keys


def _ragged_images(seed=SEED):
    rng = np.random.default_rng(seed)
    images = []
    for b, (khw, up, crop) in enumerate(RAGGED):
        rw = (rng.random(khw) ** 2).astype(np.float32)  # non-negative, like a random walk's output
        if b == 0:
            rw[1, 8, 10] = 3.0  # reaches its full height only in rows >= 34 / columns >= 42 of the 36 x 44 map
        if b == ZERO_IMAGE:
            rw[:] = 0
        images.append((rw, up, crop))
    return images


def _finish(ctx, images, keys_per_image, has_bg, thr):
    """One wsc_sem_seg_finish call over `images` [(rw float32 [K][h][w], up, crop)] -> the uint8 label map of each.  The maps
    are packed with a gap of large values between the images (an offset taken from anywhere but rw_off reads it) and the
    label buffer carries guard bytes behind the last image."""
    gap = np.full(3, 1e9, np.float32)
    parts, off, pos = [], [], 0
    for rw, _, _ in images:
        off.append(pos)
        parts += [rw.ravel(), gap]
        pos += rw.size + gap.size
    n_out = [c[0] * c[1] for _, _, c in images]
    total = int(sum(n_out))
    rw_dev = ctx.to_device(np.concatenate(parts))
    lab_dev = ctx.to_device(np.full(total + 64, GUARD, np.uint8))
    try:
        _lib.sem_seg_finish(ctx, rw_dev, off, [rw.shape for rw, _, _ in images], [u for _, u, _ in images],
                            [c for _, _, c in images], keys_per_image, has_bg, thr, lab_dev)
        lab = ctx.to_host(lab_dev, (total + 64,), np.uint8)
    finally:
        rw_dev.free()
        lab_dev.free()
    assert (lab[total:] == GUARD).all(), "wrote behind the packed labels"
    cuts = np.cumsum([0] + n_out)
    return [lab[cuts[i]:cuts[i + 1]].reshape(images[i][2]) for i in range(len(images))]


def _assert_labels(got, want, stack, tag):
    """The comparison rule of the module docstring; -> (excluded share, mismatches among the excluded pixels)."""
    safe = ref.top_two_margin(stack) > MARGIN
    excluded = 1.0 - safe.mean()
    bad = (got != want) & safe
    inside = int(((got != want) & ~safe).sum())
    print("%s: %d pixels, excluded share %.2e (%d of them differ), mismatches outside the mask %d"
          % (tag, got.size, excluded, inside, int(bad.sum())))
    assert got.shape == want.shape
    assert excluded <= MAX_EXCLUDED, (tag, excluded)
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
    return excluded, inside


@pytest.fixture(scope="module")
def ragged():
    """The ragged batch and its float64 oracle for both values of has_bg, computed once and left unchanged."""
    images = _ragged_images()
    keys = [_keys_for(b, rw.shape[0]) for b, (rw, _, _) in enumerate(images)]
    want = {}
    for has_bg in (False, True):
        want[has_bg] = [ref.sem_seg_finish(rw, up, crop, k if has_bg else k[1:], has_bg, BG_THRES)
                        for (rw, up, crop), k in zip(images, keys)]
    # what the inputs are built for: image 0's uncropped maximum is far above its cropped one, and dividing by it moves labels
    rw, up, crop = images[0]
    full = ref.upsample_bilinear(rw, up)
    cropped = full[:, :crop[0], :crop[1]]
    assert full.max() == 3.0 and cropped.max() < 1.5
    assert ((cropped / full.max() > BG_THRES).any(0) != (cropped / cropped.max() > BG_THRES).any(0)).mean() > 0.05
    return images, keys, want


@pytest.mark.parametrize("has_bg", [False, True], ids=["nobg", "bg"])
def test_sem_seg_finish_ragged_vs_oracle(ctx, ragged, has_bg):
    """Six images of different K, source, up and crop sizes in ONE call, per pixel against the float64 oracle: packed float /
    key / label offsets, the maximum over the cropped region only, the grid-stride loop (187 500 pixels), blocks without a
    pixel, the all-zero image's first-NaN rule beside neighbours whose maxima it must not disturb.  Measured on the MI355X: 4
    (without) / 3 (with the background channel) of the 187 500-pixel image's pixels lie under the margin, none elsewhere; no
    compared pixel differs.  (Over 40 seeds the oracle alone puts 7 - 24 pixels of the two runs under the margin; SEED has 7.)"""
    images, keys, want = ragged
    got = _finish(ctx, images, [k if has_bg else k[1:] for k in keys], has_bg, BG_THRES)
    worst = 0.0
    for b, (g, (lab, stack)) in enumerate(zip(got, want[has_bg])):
        excluded, _ = _assert_labels(g, lab, stack, "image %d %s has_bg=%d" % (b, RAGGED[b], has_bg))
        worst = max(worst, excluded)
    assert (got[ZERO_IMAGE] == keys[ZERO_IMAGE][1]).all()  # keys[1] behind a background channel, the first key without
    print("sem_seg_finish ragged has_bg=%d: worst excluded share %.2e" % (has_bg, worst))


@pytest.mark.parametrize("has_bg", [False, True], ids=["nobg", "bg"])
def test_sem_seg_finish_batch_invariance(ctx, ragged, has_bg):
    """Each image of the ragged batch, called alone, gives the bits it gave inside the batch."""
    images, keys, _ = ragged
    kk = [k if has_bg else k[1:] for k in keys]
    together = _finish(ctx, images, kk, has_bg, BG_THRES)
    for b in range(len(images)):
        alone = _finish(ctx, [images[b]], [kk[b]], has_bg, BG_THRES)[0]
        assert np.array_equal(alone, together[b]), (b, int((alone != together[b]).sum()))


def test_sem_seg_finish_threshold_one_is_all_background(ctx, ragged):
    """bg_thres = 1.0: the normalised maximum is d / d == 1.0, which is not > 1.0 -- every pixel is keys[0], the one holding
    the maximum included (a `>=` fails here).  No mask: nothing is rounded.  The all-zero image keeps its NaN rule."""
    images, keys, _ = ragged
    got = _finish(ctx, images, keys, True, 1.0)
    for b, g in enumerate(got):
        expect = keys[b][1] if b == ZERO_IMAGE else keys[b][0]
        assert (g == expect).all(), (b, np.unique(g).tolist(), expect)
        lab, _ = ref.sem_seg_finish(*images[b], keys[b], True, 1.0)
        assert np.array_equal(g, lab)


@pytest.mark.parametrize("has_bg", [False, True], ids=["nobg", "bg"])
def test_sem_seg_finish_identical_maps_first_key(ctx, has_bg):
    """Map 2 holds map 0's bits: the first maximum wins, so map 2's key never appears and the labels are those of the call
    without map 2.  Exact, no mask."""
    rng = np.random.default_rng(5)
    a, b = ((rng.random((9, 11)) ** 2).astype(np.float32) for _ in range(2))
    up, crop = (36, 44), (33, 41)
    keys3, keys2 = [7, 60, 61, 255], [7, 60, 61]
    if not has_bg:
        keys3, keys2 = keys3[1:], keys2[1:]
    three = _finish(ctx, [(np.stack([a, b, a]), up, crop)], [keys3], has_bg, BG_THRES)[0]
    two = _finish(ctx, [(np.stack([a, b]), up, crop)], [keys2], has_bg, BG_THRES)[0]
    assert not (three == 255).any()
    assert (three == 60).any() and (three == 61).any()
    assert np.array_equal(three, two)


@pytest.mark.parametrize("thr", [0.05, 0.25, 0.5, 0.9])
def test_sem_seg_finish_single_map_threshold(ctx, thr):
    """K = 1 behind a background channel: the label is background exactly where u / max <= bg_thres, which probes the
    normalised VALUES (the crop's maximum, the division) through a label-only output.  Up-sized, then cropped."""
    thr = float(np.float32(thr))
    rng = np.random.default_rng(6)
    rw = (rng.random((1, 24, 32)) ** 2).astype(np.float32)
    rw[0, 23, 31] = 2.5  # the uncropped maximum, removed by the crop
    up, crop, keys = (94, 125), (90, 120), [0, 255]
    got = _finish(ctx, [(rw, up, crop)], [keys], True, thr)[0]
    lab, stack = ref.sem_seg_finish(rw, up, crop, keys, True, thr)
    assert np.array_equal(lab == 0, stack[1] <= thr)
    assert 0.005 < (lab == 0).mean() < 0.995  # the threshold cuts through the image
    _assert_labels(got, lab, stack, "single map thr=%g" % thr)


# ---- wsc_label_unary_from_cam ---------------------------------------------------------------------------------------------------
THRES, GT_PROB = 0.3, 0.7
UNARY_SHAPES = [(2, 1, 1), (3, 4, 47 * 59), (1, 20, 1000), (2, 1, 1050000)]  # the last: 2 100 000 pixels > 8192 x 256


def _unary_inputs(B, K, N):
    rng = np.random.default_rng(B * 100 + K)
    maps = rng.random((B, K, N), dtype=np.float32)
    t = np.float32(THRES)
    if N == 1:
        maps[0] = t      # equal to the threshold: label 0
        maps[-1] = 0.9
    else:
        maps[:, :, 0] = t                      # every map equal to the threshold: label 0
        maps[:, :, 1] = t * np.float32(0.5)    # everything below it: label 0
        maps[:, :, 2] = t
        maps[:, 0, 2] = maps[:, K - 1, 2] = 0.9  # the first and the last map equal and above it: label 1
        maps[:, :, N - 1] = 0.1
        maps[:, K - 1, N - 1] = np.nextafter(t, np.float32(1))  # one ulp above the threshold in the last map of the last pixel
    return maps


def _label_unary(ctx, maps, want_labels):
    B, K, N = maps.shape
    m_dev = ctx.to_device(maps)
    u_dev = ctx.to_device(np.full(B * (K + 1) * N + 16, -1.0, np.float32))
    l_dev = ctx.to_device(np.full(B * N + 16, -1, np.int32)) if want_labels else None
    try:
        _lib.label_unary_from_cam(ctx, m_dev, B, K, N, THRES, GT_PROB, u_dev, l_dev)
        U = ctx.to_host(u_dev, (B * (K + 1) * N + 16,), np.float32)
        L = ctx.to_host(l_dev, (B * N + 16,), np.int32) if want_labels else None
    finally:
        for d in (m_dev, u_dev, l_dev):
            if d is not None:
                d.free()
    assert (U[-16:] == -1.0).all() and (L is None or (L[-16:] == -1).all()), "wrote behind the output"
    return U[:-16].reshape(B, K + 1, N), (None if L is None else L[:-16].reshape(B, N))


@pytest.mark.parametrize("shape", UNARY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_unary_from_cam_vs_oracle(ctx, shape):
    """Labels EQUAL to np.argmax(np.pad(...)) (a comparison of float32 numbers: nothing is rounded), every energy within one
    fp32 ulp of unary_from_labels', with and without the labels output."""
    B, K, N = shape
    maps = _unary_inputs(B, K, N)
    want = [ref.label_unary_from_cam(maps[b], THRES, GT_PROB) for b in range(B)]
    wl, wu = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    worst = 0
    for want_labels in (True, False):
        U, L = _label_unary(ctx, maps, want_labels)
        if want_labels:
            bad = L != wl
            assert not bad.any(), (shape, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        ulps = np.abs(U.view(np.int32).astype(np.int64) - wu.view(np.int32))
        worst = max(worst, int(ulps.max()))
        assert ulps.max() <= 1, (shape, want_labels, int(ulps.max()), np.argwhere(ulps > 1)[:4].tolist())
    assert len(np.unique(wl)) == min(K + 1, B * N)  # every label occurs
    print("label_unary_from_cam %s: labels equal, worst unary error %d ulp" % (shape, worst))


def test_label_unary_from_cam_edges(ctx):
    """Written out: a value equal to thres is not above it (label 0), of two equal maps above it the lower index wins, all below
    gives 0, one ulp above thres is above it."""
    t = np.float32(THRES)
    up1 = np.nextafter(t, np.float32(1))
    #                 ==thres  tie 1/3  below   1 ulp   tie 2/3 above a lower map 1
    maps = np.array([[[t,      0.8,     0.0,    t,      0.4],
                      [t,      0.5,     0.29,   up1,    0.6],
                      [t,      0.8,     0.1,    t,      0.6]]], np.float32)
    U, L = _label_unary(ctx, maps, True)
    assert L[0].tolist() == [0, 1, 0, 2, 2]
    wl, wu = ref.label_unary_from_cam(maps[0], THRES, GT_PROB)
    assert np.array_equal(L[0], wl)
    assert np.abs(U[0].view(np.int32).astype(np.int64) - wu.view(np.int32)).max() <= 1


# ---- wsc_ir_label_combine -------------------------------------------------------------------------------------------------------
def _combine_inputs(B, M, N, voc, seed):
    rng = np.random.default_rng(seed)
    keys = np.zeros((B, M), np.int32)
    for b in range(B):  # different keys per image
        cls = np.sort(rng.choice(np.arange(1, 254), M - 1, replace=False))
        keys[b] = np.pad(cls + 1, (1, 0)) if voc else np.concatenate([[-1], cls])
    keys[0, -1] = 255               # uint8's last value (voc12: class 254 + 1)
    if not voc and M > 2:
        keys[B - 1, 1] = 0          # ADP / DeepGlobe: class id 0 is a real class, not the background
    fg = rng.integers(0, M, (B, N)).astype(np.int32)
    bg = rng.integers(0, M, (B, N)).astype(np.int32)
    if B * N >= 4:  # all four (fg == 0, bg == 0) combinations, whatever the draw
        fg.reshape(-1)[:4] = [0, 0, 1, 1]
        bg.reshape(-1)[:4] = [0, 1, 0, 1]
        fg.reshape(-1)[-4:] = [1, 0, 1, 0]
        bg.reshape(-1)[-4:] = [1, 1, 0, 0]
    return keys, fg, bg


COMBINE_SHAPES = [(3, 4, 47 * 59), (1, 2, 1000), (3, 3, 1), (4, 3, 1), (1, 5, 1), (3, 5, 700001)]  # the last: B N > 8192 x 256


@pytest.mark.parametrize("voc", [True, False], ids=["voc", "adp"])
@pytest.mark.parametrize("shape", COMBINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ir_label_combine_vs_oracle(ctx, shape, voc):
    """conf = keys[fg] and the reference's assignment lines, exactly, with the keys of each image of the batch its own."""
    B, M, N = shape
    keys, fg, bg = _combine_inputs(B, M, N, voc, B * 7 + M)
    want = np.stack([ref.ir_label_combine(fg[b], bg[b] if voc else None, keys[b]) for b in range(B)])
    if B * N >= 4:
        seen = {(bool(f == 0), bool(g == 0)) for f, g in zip(fg.reshape(-1)[:4], bg.reshape(-1)[:4])}
        assert len(seen) == 4
    fg_dev, bg_dev = ctx.to_device(fg), (ctx.to_device(bg) if voc else None)
    c_dev = ctx.to_device(np.full(B * N + 64, GUARD, np.uint8))
    try:
        _lib.ir_label_combine(ctx, fg_dev, bg_dev, keys, N, c_dev)
        got = ctx.to_host(c_dev, (B * N + 64,), np.uint8)
    finally:
        for d in (fg_dev, bg_dev, c_dev):
            if d is not None:
                d.free()
    assert (got[B * N:] == GUARD).all()
    got = got[:B * N].reshape(B, N)
    bad = got != want
    print("ir_label_combine %s %s: %d of %d pixels differ" % (shape, "voc" if voc else "adp", int(bad.sum()), bad.size))
    assert not bad.any(), (shape, voc, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def test_ir_label_combine_single_pixels_cover_all_cases(ctx):
    """N = 1, B = 4: one (fg == 0, bg == 0) combination per image."""
    keys = np.array([[0, 3], [0, 9], [0, 255], [0, 17]], np.int32)
    fg = np.array([[0], [0], [1], [1]], np.int32)
    bg = np.array([[0], [1], [0], [1]], np.int32)
    fg_dev, bg_dev, c_dev = ctx.to_device(fg), ctx.to_device(bg), ctx.alloc(4)
    _lib.ir_label_combine(ctx, fg_dev, bg_dev, keys, 1, c_dev)
    assert ctx.to_host(c_dev, (4,), np.uint8).tolist() == [0, 255, 255, 17]
    keys[:, 0] = -1
    _lib.ir_label_combine(ctx, fg_dev, None, keys, 1, c_dev)
    assert ctx.to_host(c_dev, (4,), np.uint8).tolist() == [255, 255, 255, 17]
    for d in (fg_dev, bg_dev, c_dev):
        d.free()


# ---- wsc_cam_sum_scales ---------------------------------------------------------------------------------------------------------
def _scale_maps(rng, n, elems):
    """Magnitudes six decades apart: the order of the float32 additions shows in the bits."""
    return (rng.normal(0, 1, (n, elems)) * 10.0 ** rng.uniform(-3, 3, (n, elems))).astype(np.float32)


def _sum_scales(ctx, cam, n_images, n_scales, elems):
    cam_dev = ctx.to_device(cam)
    out_dev = ctx.to_device(np.full(n_images * elems + 16, -7.0, np.float32))
    try:
        _lib.cam_sum_scales(ctx, cam_dev, n_images, n_scales, elems, out_dev)
        out = ctx.to_host(out_dev, (n_images * elems + 16,), np.float32)
    finally:
        cam_dev.free()
        out_dev.free()
    assert (out[-16:] == -7.0).all()
    return out[:-16].reshape(n_images, elems)


@pytest.mark.parametrize("n_images,n_scales,elems", [(3, 1, 1001), (3, 2, 1001), (2, 3, 21 * 21 * 5), (3, 5, 1001), (1, 2, 1),
                                                     (3, 2, 700001)])  # the last: 2 100 003 sums > 8192 x 256
def test_cam_sum_scales_bit_identical(ctx, n_images, n_scales, elems):
    rng = np.random.default_rng(n_scales * 10 + n_images)
    cam = _scale_maps(rng, n_images * n_scales, elems)
    want = ref.cam_sum_scales(cam, n_scales)
    got = _sum_scales(ctx, cam, n_images, n_scales, elems)
    bad = got.view(np.int32) != want.view(np.int32)
    print("cam_sum_scales %d x %d x %d: %d of %d sums differ in their bits" % (n_images, n_scales, elems, int(bad.sum()), bad.size))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
    if n_scales >= 3 and elems > 1000:  # the inputs do tell one order from another
        other = ref.cam_sum_scales(np.ascontiguousarray(cam.reshape(n_images, n_scales, elems)[:, ::-1]).reshape(-1, elems), n_scales)
        assert (other.view(np.int32) != want.view(np.int32)).any()


def test_cam_sum_scales_in_place(ctx):
    """One scale may be 'summed' in place (a copy onto itself); several scales in place would read what they overwrite and
    are refused with WSC_ERR_INVALID, the buffer untouched."""
    rng = np.random.default_rng(1)
    cam = _scale_maps(rng, 4, 333)
    dev = ctx.to_device(cam)
    try:
        _lib.cam_sum_scales(ctx, dev, 4, 1, 333, dev)
        assert np.array_equal(ctx.to_host(dev, cam.shape, np.float32).view(np.int32), cam.view(np.int32))
        with pytest.raises(_lib.WscError) as e:
            _lib.cam_sum_scales(ctx, dev, 2, 2, 333, dev)
        assert e.value.status == _lib.WSC_ERR_INVALID
        assert np.array_equal(ctx.to_host(dev, cam.shape, np.float32).view(np.int32), cam.view(np.int32))
    finally:
        dev.free()


# ---- wsc_hsn_voc_background / wsc_hsn_class_mass --------------------------------------------------------------------------------
HSN_TOL = 2e-6  # test_gpu_hsn.py's bound for the element-wise stages
SENTINEL = -7.0


def _voc_background(ctx, Hbg, Ctot):
    B, Cb, N = Hbg.shape
    h_dev = ctx.to_device(Hbg)
    y_dev = ctx.to_device(np.full(B * Ctot * N + 16, SENTINEL, np.float32))
    try:
        _lib.hsn_voc_background(ctx, h_dev, B, Cb, N, y_dev, Ctot)
        y = ctx.to_host(y_dev, (B * Ctot * N + 16,), np.float32)
    finally:
        h_dev.free()
        y_dev.free()
    assert (y[-16:] == SENTINEL).all()
    y = y[:-16].reshape(B, Ctot, N)
    assert (y[:, 1:] == SENTINEL).all(), "channels other than 0 were written"
    return y[:, 0]


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 57 * 57), (6, 2, 321 * 321)],  # the last: 618 246 sums > 2048 x 256
                         ids=lambda s: "x".join(map(str, s)))
def test_hsn_voc_background_vs_oracle(ctx, shape):
    """0.15 * expit(max over the WHOLE batch - X_bg) into channel 0 of a wider stack.  The batch maximum sits in the last image
    (a per-image maximum is off by O(0.1) in every other image); the other channels keep their sentinel."""
    B, Cb, N = shape
    rng = np.random.default_rng(B + Cb)
    Hbg = (rng.random(shape) ** 2).astype(np.float32)
    Hbg[B - 1, :, N - 1] = 1.5  # X_bg = 1.5 Cb at the last pixel of the last image: above Cb, the bound of every other sum
    want = ref.hsn_voc_background(Hbg)
    if B > 1:
        X = Hbg.astype(np.float64).sum(1)
        assert X[:-1].max() < X.max() - 0.4
    got = _voc_background(ctx, Hbg, 3)
    err = np.abs(got - want).max()
    print("hsn_voc_background %s: worst |error| %.3g (bound %.0e)" % (shape, err, HSN_TOL))
    assert err <= HSN_TOL, (shape, err)


def test_hsn_voc_background_all_zero(ctx):
    got = _voc_background(ctx, np.zeros((2, 3, 57 * 57), np.float32), 2)
    err = np.abs(got.astype(np.float64) - 0.075).max()
    print("hsn_voc_background all zero: worst |error| %.3g" % err)
    assert err <= HSN_TOL


def test_hsn_class_mass_exact(ctx):
    """N = 321 x 321 > 64 blocks x 256 threads: a map whose only positive entry is its last pixel, one whose only positive entry
    is its first, and an all-zero map between two positive ones."""
    N = 321 * 321
    rng = np.random.default_rng(9)
    maps = np.zeros((6, N), np.float32)
    maps[0, N - 1] = 1e-30
    maps[1, 0] = 1e-30
    maps[2] = rng.random(N, dtype=np.float32)
    maps[4] = rng.random(N, dtype=np.float32)
    maps[5, 64 * 256 + 3] = 0.5  # only the second trip of the grid-stride loop sees it
    want = ref.class_mass(maps)
    assert want.tolist() == [True, True, True, False, True, True]
    m_dev = ctx.to_device(maps)
    mass_dev = ctx.to_device(np.full(8, 77, np.uint32))
    try:
        _lib.hsn_class_mass(ctx, m_dev, 6, N, mass_dev)
        mass = ctx.to_host(mass_dev, (8,), np.uint32)
    finally:
        m_dev.free()
        mass_dev.free()
    print("hsn_class_mass:", mass[:6].tolist())
    assert mass[6:].tolist() == [77, 77]
    assert mass[:6].tolist() == want.astype(np.uint32).tolist()


# ---- wsc_bilinear_resize: DeepGlobe's / 6 branch (make_sem_seg_labels.py:101-104) ------------------------------------------------
@pytest.mark.parametrize("chw,size", [((3, 50, 73), (8, 12)), ((1, 7, 6), (1, 1))], ids=["50x73-8x12", "7x6-1x1"])
def test_bilinear_resize_downsize(ctx, chw, size):
    """An output SMALLER than the source (scale > 1: the taps skip source pixels, no antialiasing): 2e-6 against torch's
    fp32 F.interpolate, 1e-5 against the float64 oracle."""
    rng = np.random.default_rng(chw[1])
    x = rng.random(chw, dtype=np.float32)
    C, h, w = chw
    src_dev, dst_dev = ctx.to_device(x), ctx.alloc(C * size[0] * size[1] * 4)
    try:
        _lib.bilinear_resize(ctx, src_dev, C, h, w, dst_dev, size[0], size[1])
        got = ctx.to_host(dst_dev, (C,) + size, np.float32)
    finally:
        src_dev.free()
        dst_dev.free()
    t32 = F.interpolate(torch.from_numpy(x)[None], size=size, mode="bilinear", align_corners=False)[0].numpy()
    e32 = np.abs(got - t32).max()
    e64 = np.abs(got - ref.upsample_bilinear(x, size)).max()
    print("bilinear_resize %s -> %s: %.3g vs torch fp32 (2e-6), %.3g vs float64 (1e-5)" % (chw, size, e32, e64))
    assert e32 <= 2e-6 and e64 <= 1e-5, (e32, e64)
