"""numpy restatement of the IRNet training-sample transform (03b_irn/voc12/dataloader.py:270-321 and its ADP / DeepGlobe twins):
PIL's resample (bicubic, 8 bits per channel) and nearest rescale, the float64 bilinear of TorchvisionResize, normalise, flip,
crop with padding, HWC -> CHW and the quarter-size nearest reduction of the label.  Written from the published algorithms
(Pillow's Resample.c / Geometry.c), independent of wsscam; needs no PIL.  tests/test_irn_batch_oracle.py pins the two resamples
against Image.resize itself.

A parameter record is the 9-tuple (scaled_h, scaled_w, flip, cont_top, cont_left, img_top, img_left, ch, cw)."""
import numpy as np

PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resample_coeffs(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for the bicubic filter (support 2): per output index
    (xmin, n, int32 coefficients [n])."""
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    out = []
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:  # the sum in index order
            ww += v
        if ww != 0.0:
            w = w / ww
        coef = np.array([int(v * (1 << PRECISION_BITS) + (-0.5 if v < 0 else 0.5)) for v in w], np.int64)
        out.append((xmin, n, coef))
    return out


def _resample_axis0(img, out_size):
    """one pass of ImagingResample along axis 0 of a uint8 array (any trailing axes)"""
    tab = resample_coeffs(img.shape[0], out_size)
    v = img.astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for i, (xmin, n, coef) in enumerate(tab):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coef, v[xmin:xmin + n], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_bicubic(img, out_hw):
    """Image.resize((w, h), BICUBIC) of a uint8 (H, W) or (H, W, C) array: the horizontal pass, then the vertical pass on its
    uint8 result; a pass whose axis keeps its size is skipped."""
    img = np.ascontiguousarray(img, np.uint8)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if ow != img.shape[1]:
        img = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), ow), 0, 1)
    if oh != img.shape[0]:
        img = _resample_axis0(img, oh)
    return np.ascontiguousarray(img)


def nearest_index(in_size, out_size):
    """ImagingScaleAffine's source index per output index: the running sum in double, not i * a"""
    a = np.float64(in_size) / np.float64(out_size)
    v = a * 0.5
    idx = np.empty(out_size, np.int64)
    for i in range(out_size):
        idx[i] = int(v)
        v += a
    return idx


def pil_nearest(img, out_hw):
    """Image.resize((w, h), NEAREST)"""
    img = np.ascontiguousarray(img, np.uint8)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    return np.ascontiguousarray(img[nearest_index(img.shape[0], oh)][:, nearest_index(img.shape[1], ow)])


def pil_resize(img, out_hw, order):
    """misc.imutils.pil_resize: the array itself when the size is right"""
    if (int(out_hw[0]), int(out_hw[1])) == tuple(img.shape[:2]):
        return img
    return pil_bicubic(img, out_hw) if order == 3 else pil_nearest(img, out_hw)


def scaled_size(hw, factor):
    """the target of misc.imutils.pil_rescale"""
    return int(np.round(hw[0] * factor)), int(np.round(hw[1] * factor))


def reduced_size(S):
    return int(np.round(S * 0.25))


def bilinear_f64(img, out_hw):
    """TorchvisionResize: np.asarray(img, 'float64'), cv2.resize (INTER_LINEAR, half-pixel centres) where the size differs"""
    H, W = img.shape[:2]
    oh, ow = int(out_hw[0]), int(out_hw[1])
    im = np.asarray(img, np.float64)
    if (H, W) == (oh, ow):
        return im
    out = np.empty((oh, ow) + im.shape[2:], np.float64)
    for y in range(oh):
        fy = min(max((y + 0.5) * H / oh - 0.5, 0.0), float(H - 1))
        y0 = int(fy)
        y1 = min(y0 + 1, H - 1)
        wy = fy - y0
        for x in range(ow):
            fx = min(max((x + 0.5) * W / ow - 0.5, 0.0), float(W - 1))
            x0 = int(fx)
            x1 = min(x0 + 1, W - 1)
            wx = fx - x0
            top = im[y0, x0] * (1.0 - wx) + im[y0, x1] * wx
            bot = im[y1, x0] * (1.0 - wx) + im[y1, x1] * wx
            out[y, x] = top * (1.0 - wy) + bot * wy
    return out


def normalise(img, mean, std, pre_div255):
    """TorchvisionNormalize: one float32 subtract and one float32 divide per value, a divide by 255 first in 'float' mode"""
    f = np.asarray(img).astype(np.float32)
    out = np.empty(f.shape, np.float32)
    for c in range(3):
        v = f[..., c]
        if pre_div255:
            v = v / np.float32(255.0)
        out[..., c] = (v - np.float32(mean[c])) / np.float32(std[c])
    return out


def crop(img, S, fill, box):
    cont_top, cont_left, img_top, img_left, ch, cw = box
    out = np.full((S, S) + img.shape[2:], fill, img.dtype)
    out[cont_top:cont_top + ch, cont_left:cont_left + cw] = img[img_top:img_top + ch, img_left:img_left + cw]
    return out


def transform(img, label, params, S, mean, std, pre_div255, stage):
    """One sample: uint8 (H, W, 3) image and (H, W) label -> (x float32 (3, S, S), label uint8 (S, S), reduced uint8 (s, s)).
    stage 0: no resize; 1: the PIL rescale to scaled_h x scaled_w; 2: TorchvisionResize to scaled_h x scaled_w, the label too,
    truncated to uint8."""
    sh, sw, flip = int(params[0]), int(params[1]), int(params[2])
    box = tuple(int(v) for v in params[3:9])
    if stage == 1:
        img = pil_resize(img, (sh, sw), 3)
        label = pil_resize(label, (sh, sw), 0)
    elif stage == 2:
        img = bilinear_f64(img, (sh, sw))
        label = bilinear_f64(label, (sh, sw))
    assert tuple(img.shape[:2]) == (sh, sw) == tuple(label.shape[:2])
    x = normalise(img, mean, std, pre_div255)
    if flip:
        x, label = np.fliplr(x), np.fliplr(label)
    x = crop(x, S, np.float32(0.0), box)
    label = crop(label, S, 255, box).astype(np.uint8)  # (np.uint8 of the float64 label: truncation)
    s = reduced_size(S)
    reduced = pil_nearest(label, (s, s))
    return np.ascontiguousarray(np.transpose(x, (2, 0, 1))), label, reduced


def batch(images, labels, params, S, mean, std, pre_div255, stage):
    outs = [transform(i, l, p, S, mean, std, pre_div255, stage) for i, l, p in zip(images, labels, params)]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))
