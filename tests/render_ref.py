"""numpy oracle of the debug-image renderer, written as the reference writes it (03c_hsn/demo.py:181-199, :394-418;
02_cues/demo.py:433-477): the per-class `pred_segmask += mask * colour` loop on a float64 array, np.uint8(...), the literal
blend expressions, and cv2's INTER_NEAREST restated from include/wsscam.h (wsc_cam_eval_confusion_nn):
    src = min(floor(x * (1. / (out / src_size))), src_size - 1)   in double
This module knows nothing of wsscam.render and uses no blend table."""
import numpy as np


def nearest_index(src, out):
    """Source index of every output index of cv2.resize(..., INTER_NEAREST) along one axis."""
    inv = 1.0 / (float(out) / float(src))
    return np.minimum(np.floor(np.arange(out, dtype=np.float64) * inv).astype(np.int64), src - 1)


def resize_nearest(a, out_hw):
    """cv2.resize(a, (out_w, out_h), interpolation=cv2.INTER_NEAREST) of an (h, w) or (h, w, c) array."""
    a = np.asarray(a)
    return a[nearest_index(a.shape[0], out_hw[0])][:, nearest_index(a.shape[1], out_hw[1])]


def segmask(pred_idx, colours, other_rgb=(0, 0, 0)):
    """The reference's loop: pred_segmask = zeros((H, W, 3)); for k: pred_segmask += (pred_idx == k)[..., None] * colours[k] --
    float64.  A label no class claims stays at zero in the reference; `other_rgb` puts a colour there (03a's label2rgb: white)."""
    pred_idx = np.asarray(pred_idx)
    colours = np.asarray(colours)
    pred_segmask = np.zeros(pred_idx.shape + (3,))
    listed = np.zeros(pred_idx.shape, dtype=bool)
    for k in range(len(colours)):
        pred_mask = pred_idx == k
        pred_segmask += np.expand_dims(pred_mask, axis=2) * np.expand_dims(np.expand_dims(colours[k], axis=0), axis=0)
        listed |= pred_mask
    pred_segmask += np.expand_dims(~listed, axis=2) * np.expand_dims(np.expand_dims(np.asarray(other_rgb), axis=0), axis=0)
    return pred_segmask


def float_to_byte(x):
    """What imsave makes of a float image in [0, 1]: rint(x * 255) (ties to even), clipped to a byte."""
    return np.uint8(np.clip(np.rint(np.asarray(x, dtype=np.float64) * 255), 0, 255))


def render(labels, colours, out_hw, mid_hw=None, other_rgb=(0, 0, 0), img=None, overlay_r=0.75, rule="uint8"):
    """(colour image, overlay or None) of one label map.  The nearest stages act on the label map: a nearest resize only picks
    pixels, so it commutes with the per-pixel colouring (the reference resizes the label map first, :181 / :394, and the
    coloured float image second, :411)."""
    pred_idx = np.asarray(labels)
    if mid_hw is not None:
        pred_idx = resize_nearest(pred_idx, mid_hw)
    pred_idx = resize_nearest(pred_idx, out_hw)
    pred_segmask = segmask(pred_idx, colours, other_rgb)
    OVERLAY_R = overlay_r
    if rule == "uint8":
        colour = np.uint8(pred_segmask)
        over = None if img is None else np.uint8((1 - OVERLAY_R) * img + OVERLAY_R * pred_segmask)
    else:
        assert rule == "float256"
        colour = float_to_byte(pred_segmask / 256.0)
        over = None if img is None else float_to_byte((1 - OVERLAY_R) * img / 256.0 + OVERLAY_R * pred_segmask / 256.0)
    return colour, over
