"""numpy restatement of the 01_train sample transform (csrc/cls_batch.hip, wsc_cls_train_batch): what Keras' ImageDataGenerator
behind flow_from_dataframe(target_size=(H, W)) does to one decoded uint8 RGB image, step by step --

  1. load_img(target_size): PIL Image.resize((W, H), NEAREST), skipped when the image has that size (tests/irn_batch_ref.py's
     nearest_index: ImagingScaleAffine's running sum);
  2. scipy.ndimage.affine_transform(plane, M, off, order=1, mode, cval) on each float32 H x W plane (ni_interpolation.c,
     NI_GeometricTransform), restated in float64:
        c_k = 0; c_k += r * M[k][0]; c_k += col * M[k][1]; c_k += off[k]   (k = 0 the row axis: the matrix product first, the
                                                                           offset last)
        c_k = map_coordinate(c_k, n_k, mode); c_k <= -1 in any axis: the pixel is cval
        start = floor(c_k), f = c_k - floor(c_k), weights (1 - f, 1 - (1 - f)) -- the last weight is one minus the others --,
        both tap indices start, start + 1 mapped by the mode again (integer reflection; a clamp for nearest AND constant)
        t = 0; for i, j in row-major order: t += (v[i][j] * wy[i]) * wx[j]; one rounding to float32 at the end;
  3. flip_axis on the columns and / or rows, after the warp;
  4. standardize: preprocessing_function, then rescale: y = ((v - sub[c]) / div) * mul, every operation one float32 rounding;
  5. HWC -> CHW, the channels stay R, G, B.

tests/test_cls_batch_oracle.py pins this file against PIL and scipy themselves, bit for bit; the device is held against this file."""
import numpy as np

from tests import irn_batch_ref

MODES = {"nearest": 0, "reflect": 1, "constant": 2}
FLAG_WARP, FLAG_FLIP_COLS, FLAG_FLIP_ROWS = 1, 2, 4

# (sub3, div, mul) of the three datasets' normalize() + rescale (02_cues/dataset.py:28-96)
STANDARDISE = {
    "ADP": ((193.09203, 193.09203, 193.09203), np.float32(56.450138 + 1e-7), np.float32(1.0)),
    "VOC2012": ((104.0, 117.0, 123.0), np.float32(1.0), np.float32(1.0 / 255)),
    "DeepGlobe": ((0.0, 0.0, 0.0), np.float32(1.0), np.float32(1.0 / 255)),
}


def _trunc(x):
    """(npy_intp) of a double, back as a double"""
    return np.trunc(x)


def map_coordinate(c, n, mode):
    """map_coordinate of ni_interpolation.c on a float64 array, for an axis of n samples; a constant-mode coordinate outside
    [0, n - 1] becomes -1"""
    c = np.array(c, np.float64, copy=True)
    lo, hi = c < 0, c > n - 1
    if mode == "nearest":
        c[lo] = 0.0
        c[hi] = n - 1
    elif mode == "constant":
        c[lo | hi] = -1.0
    elif mode == "reflect":
        if n <= 1:
            c[lo | hi] = 0.0
            return c
        sz2 = np.float64(2 * n)
        v = c[lo]
        far = v < -sz2
        v[far] = sz2 * _trunc(-v[far] / sz2) + v[far]
        v = np.where(v < -n, v + sz2, np.where(v > -1e-15, 1e-15, -v) - 1)
        c[lo] = v
        v = c[hi]
        v = v - sz2 * _trunc(v / sz2)
        v = np.where(v >= n, sz2 - v - 1, v)
        c[hi] = v
    else:
        raise ValueError("mode %r" % (mode,))
    return c


def map_index(i, n, mode):
    """the border mapping of a tap index (int64 array)"""
    i = np.array(i, np.int64, copy=True)
    if n <= 1:
        return np.zeros_like(i)
    if mode in ("nearest", "constant"):
        return np.clip(i, 0, n - 1)
    s2 = 2 * n
    neg = i < 0
    v = i[neg]
    far = v < -s2
    v[far] = s2 * ((-v[far]) // s2) + v[far]
    i[neg] = np.where(v < -n, v + s2, -v - 1)
    big = i >= n
    v = i[big]
    v = v - s2 * (v // s2)
    i[big] = np.where(v >= n, s2 - v - 1, v)
    return i


def warp_plane(plane, affine, mode, cval):
    """scipy.ndimage.affine_transform(plane, [[M00, M01], [M10, M11]], (off0, off1), order=1, mode=mode, cval=cval) of a float32
    (H, W) plane; affine = (M00, M01, M10, M11, off0, off1) doubles"""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    a = np.asarray(affine, np.float64)
    r = np.arange(H, dtype=np.float64)[:, None]
    col = np.arange(W, dtype=np.float64)[None, :]
    coords = []
    for k, n in ((0, H), (1, W)):
        c = np.zeros((H, W), np.float64)
        c = c + r * a[2 * k]
        c = c + col * a[2 * k + 1]
        c = c + a[4 + k]
        coords.append(map_coordinate(c, n, mode))
    outside = (coords[0] <= -1.0) | (coords[1] <= -1.0)
    taps = []
    for c, n in zip(coords, (H, W)):
        fl = np.floor(c)
        f = c - fl
        w0 = 1.0 - f
        w1 = 1.0 - w0
        s = fl.astype(np.int64)
        taps.append(((map_index(s, n, mode), map_index(s + 1, n, mode)), (w0, w1)))
    v = plane.astype(np.float64)
    t = np.zeros((H, W), np.float64)
    for i in range(2):
        for j in range(2):
            t = t + (v[taps[0][0][i], taps[1][0][j]] * taps[0][1][i]) * taps[1][1][j]
    t[outside] = np.float64(cval)
    return t.astype(np.float32)


def standardise(x, sub3, div, mul):
    """float32 (H, W, 3) -> ((x - sub[c]) / div) * mul, one float32 rounding per operation"""
    x = np.asarray(x, np.float32)
    sub = np.asarray(sub3, np.float32).reshape(1, 1, 3)
    return ((x - sub) / np.float32(div)) * np.float32(mul)


def sample(img, hw, affine, flags, mode, cval, sub3, div, mul):
    """uint8 (H0, W0, 3) -> float32 (3, H, W)"""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = int(hw[0]), int(hw[1])
    if img.shape[:2] != (H, W):
        img = irn_batch_ref.pil_nearest(img, (H, W))
    x = img.astype(np.float32)
    if flags & FLAG_WARP:
        x = np.stack([warp_plane(x[:, :, c], affine, mode, np.float32(cval)) for c in range(3)], axis=2)
    if flags & FLAG_FLIP_COLS:
        x = x[:, ::-1]
    if flags & FLAG_FLIP_ROWS:
        x = x[::-1]
    return np.ascontiguousarray(standardise(x, sub3, div, mul).transpose(2, 0, 1))


def batch(images, hw, affines, flags, mode, cval, sub3, div, mul):
    """-> float32 (B, 3, H, W)"""
    return np.stack([sample(im, hw, a, int(f), mode, cval, sub3, div, mul) for im, a, f in zip(images, affines, flags)])


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------
TARGETS = ((1, 1), (3, 5), (8, 8), (17, 33))
SOURCES = ((1, 1), (5, 23), (16, 16), (40, 31))
CVALS = (0.0, 37.5)
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def sources_for(hw):
    """the four source sizes and the target itself (no resize)"""
    return SOURCES + ((int(hw[0]), int(hw[1])),)


def image(seed, hw):
    return np.random.RandomState(seed).randint(0, 256, (int(hw[0]), int(hw[1]), 3)).astype(np.uint8)


def six(m):
    """Keras' 3 x 3 transform matrix -> M00 M01 M10 M11 off0 off1 (final_affine_matrix, final_offset)"""
    return (m[0, 0], m[0, 1], m[1, 0], m[1, 1], m[0, 2], m[1, 2])


def named_affines(H, W):
    """the fixed transforms of the issue: identity, an integer and a half-pixel shift, a 90 degree rotation and the zooms 0.5
    and 2 as Keras composes them about the centre, and shifts of 2.5 image widths / heights: more than one reflection period"""
    from wsscam.cls_train import ImageAugmenter

    tm = ImageAugmenter.transform_matrix
    return {
        "identity": IDENTITY,
        "shift-integer": (1.0, 0.0, 0.0, 1.0, 2.0, -3.0),
        "shift-half": (1.0, 0.0, 0.0, 1.0, 0.5, -1.5),
        "rot90": six(tm({"theta": 90.0}, H, W)),
        "zoom-0.5": six(tm({"zx": 0.5, "zy": 0.5}, H, W)),
        "zoom-2": six(tm({"zx": 2.0, "zy": 2.0}, H, W)),
        "shift-2.5-widths": six(tm({"ty": 2.5 * W}, H, W)),
        "shift-2.5-heights-back": six(tm({"tx": -2.5 * H, "ty": 0.25}, H, W)),
    }


def voc_draws(seed, H, W, count):
    """`count` transforms of the VOC2012 training generator from RandomState(seed) -> (affine (count, 6), flags (count,))"""
    from wsscam.cls_train import ImageAugmenter

    aug, rng = ImageAugmenter.for_dataset("VOC2012", True), np.random.RandomState(seed)
    affine, flags = np.zeros((count, 6), np.float64), np.zeros(count, np.int32)
    for k in range(count):
        a, flags[k] = aug.affine(aug.get_random_transform((H, W, 3), rng), H, W)
        if a is not None:
            affine[k] = a
    return affine, flags
