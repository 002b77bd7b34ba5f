"""The should_saveimg debug images of every stage: a colour-coded segmentation and its overlay on the input image, rendered on
the device by wsc_render_labels from label maps that are already there (03c_hsn/demo.py:183-199, :211-232, :395-418;
02_cues/demo.py:433-477, :604-608; 03a_sec-dsrg/model.py:596-612).

The reference builds `pred_segmask += (pred_idx == k)[..., None] * colours[k]` per class on a float64 (H, W, 3) array, resizes
it with cv2's INTER_NEAREST and blends in float64.  The per-class masks are exclusive, so the sum is one palette lookup; the
nearest resizes commute with that lookup, so they act on the label map; and the blend of two bytes is a function of (palette
entry, channel, image byte), so the host tabulates the reference's literal numpy expression once (`blend_table`) and the
device looks it up -- bit-identical with numpy for every overlay ratio, with no floating-point arithmetic on the device.

Two blend rules occur in the reference:
  "uint8"     np.uint8((1 - R) * img + R * mask) in float64 (03c_hsn, 03a_sec-dsrg, 02_cues ADP); the colour image is
              np.uint8(mask), the palette itself
  "float256"  02_cues VOC2012 / DeepGlobe (demo.py:475-477): the FLOAT images mask / 256.0 and
              (1 - R) * img / 256.0 + R * mask / 256.0 are handed to skimage's imsave, which converts a float image in [0, 1]
              to bytes.  That conversion is restated here as clip(rint(x * 255), 0, 255) (ties to even) -- skimage and imageio
              are not installed where this package was developed, so this restatement is UNPINNED against them (DESIGN.md
              section 7).  The colour image goes through the same conversion (`palette_bytes`).
"""
import os

import numpy as np

RULES = ("uint8", "float256")

# get_colours('VOC2012') of 03c_hsn/utilities.py:116-122 and 02_cues/utilities.py: the PASCAL VOC palette, background first
VOC_COLOURS = [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128), (128, 128, 128),
               (64, 0, 0), (192, 0, 0), (64, 128, 0), (192, 128, 0), (64, 0, 128), (192, 0, 128), (64, 128, 128), (192, 128, 128),
               (0, 64, 0), (128, 64, 0), (0, 192, 0), (128, 192, 0), (0, 64, 128)]


def colours_for(dataset):
    """The class colours the drivers draw with: get_colours(dataset), DeepGlobe without its last ('unknown') entry
    (03c_hsn/demo.py:90-92); 'ADP-morph' / 'ADP-func' are the ground truth's own colour tables."""
    from .step.eval_cam import ADP_CLS_COLOURS, DEEPGLOBE_CLS_COLOURS

    if dataset == "VOC2012":
        return list(VOC_COLOURS)
    if "DeepGlobe" in dataset:
        return [tuple(c) for c in DEEPGLOBE_CLS_COLOURS]
    return [tuple(int(v) for v in c) for c in ADP_CLS_COLOURS[dataset.replace("ADP-", "")]]


def _float_to_byte(x):
    """skimage's float -> uint8 of an image in [0, 1] (img_as_ubyte): rint(x * 255), ties to even, clipped.  Unpinned."""
    return np.uint8(np.clip(np.rint(np.asarray(x, dtype=np.float64) * 255), 0, 255))


def _entries(palette, other_rgb):
    pal = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    assert 1 <= len(pal) <= 63, "1 <= n_colours <= 63"
    return np.concatenate([pal, np.asarray(other_rgb, dtype=np.uint8).reshape(1, 3)])


def palette_bytes(palette, other_rgb, rule="uint8"):
    """(palette, other_rgb) as the bytes the colour image holds: themselves under "uint8" (np.uint8(pred_segmask)); under
    "float256" what imsave makes of pred_segmask / 256.0."""
    assert rule in RULES, rule
    ent = _entries(palette, other_rgb)
    if rule == "float256":
        ent = _float_to_byte(ent.astype(np.float64) / 256.0)
    return ent[:-1], ent[-1]


def blend_table(palette, other_rgb, overlay_r, rule="uint8"):
    """uint8 (n_colours + 1, 3, 256): table[e][ch][v] = the overlay byte of an image byte v under palette entry e (entry n_colours:
    other_rgb) in channel ch, by the reference's literal expression on float64 arrays."""
    assert rule in RULES, rule
    mask = _entries(palette, other_rgb).astype(np.float64)[:, :, None]  # pred_segmask is a float64 array
    img = np.arange(256, dtype=np.uint8)[None, None, :]                # orig_img is a uint8 array
    r = overlay_r
    if rule == "uint8":
        return np.ascontiguousarray(np.uint8((1 - r) * img + r * mask))
    return np.ascontiguousarray(_float_to_byte((1 - r) * img / 256.0 + r * mask / 256.0))


def render_labels(ctx, labels, sizes, out_sizes, palette, other_rgb=(0, 0, 0), *, mid_sizes=None, images=None, overlay_r=0.75,
                  rule="uint8", label_dtype=None, labels_off=None):
    """Renders a ragged batch and returns the host arrays: ([colour (H, W, 3) uint8 per image], [overlay ...] or None).

    labels     a list of (h, w) label maps on the host (uint8, or anything else as int32), or a device buffer that holds them
               (then `label_dtype` uint8 / int32 and, unless they are packed back to back in order, `labels_off` in elements)
    sizes      [(h, w)] of the label maps; out_sizes [(H, W)] of the images; mid_sizes None or [(h', w') or None]: a second
               nearest stage in between (03c_hsn/demo.py:394,411)
    images     None (no overlay), a list of uint8 (H, W, 3) RGB arrays at out_sizes, or a device buffer that holds them
               packed back to back
    palette    (n_colours, 3); a label outside [0, n_colours) takes other_rgb"""
    from . import _lib

    B = len(sizes)
    sizes = [(int(h), int(w)) for h, w in sizes]
    out_sizes = [(int(h), int(w)) for h, w in out_sizes]
    assert len(out_sizes) == B and B >= 1
    if isinstance(labels, (list, tuple)):
        label_dtype = np.uint8 if all(np.asarray(m).dtype == np.uint8 for m in labels) else np.int32
        maps = [np.ascontiguousarray(m, dtype=label_dtype) for m in labels]
        assert [m.shape for m in maps] == sizes, ([m.shape for m in maps], sizes)
        labels = ctx.to_device(np.concatenate([m.reshape(-1) for m in maps]), pooled=True)
        labels_off = None
    assert label_dtype is not None, "label_dtype: the element type of a device label buffer"
    if labels_off is None:
        labels_off = np.concatenate(([0], np.cumsum([h * w for h, w in sizes])))[:-1]
    nbytes = [3 * h * w for h, w in out_sizes]
    out_off = np.concatenate(([0], np.cumsum(nbytes))).astype(np.int64)
    total = int(out_off[-1])
    mids = None
    if mid_sizes is not None:
        mids = [(0, 0) if m is None else (int(m[0]), int(m[1])) for m in mid_sizes]
    pal, other = palette_bytes(palette, other_rgb, rule)
    colour_dev = ctx.alloc(total, pooled=True)
    img_dev = overlay_dev = blend = None
    if images is not None:
        if isinstance(images, (list, tuple)):
            ims = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
            assert [im.shape for im in ims] == [s + (3,) for s in out_sizes], ([im.shape for im in ims], out_sizes)
            img_dev = ctx.to_device(np.concatenate([im.reshape(-1) for im in ims]), pooled=True)
        else:
            img_dev = images
        overlay_dev = ctx.alloc(total, pooled=True)
        blend = blend_table(palette, other_rgb, overlay_r, rule)
    _lib.render_labels(ctx, labels, label_dtype, sizes, out_sizes, labels_off, out_off[:-1], pal, other, colour_dev, mid_sizes=mids,
                       img_dev=img_dev, blend=blend, overlay_dev=overlay_dev)

    def unpack(dev):
        flat = ctx.to_host(dev, (total,), np.uint8)
        return [flat[out_off[b]:out_off[b + 1]].reshape(out_sizes[b] + (3,)) for b in range(B)]

    return unpack(colour_dev), (unpack(overlay_dev) if overlay_dev is not None else None)


def resize_u8_grouped(ctx, images, sizes):
    """cv2.resize(image, dsize) -- 8-bit INTER_LINEAR, wsc_resize_u8; a copy at equal sizes -- of every image to its own
    (height, width), the images of one target size in one call (one upload, one launch, one download per distinct size)."""
    from .cues.demo import read_batch_u8

    out, groups = [None] * len(images), {}
    for b, hw in enumerate(sizes):
        groups.setdefault((int(hw[0]), int(hw[1])), []).append(b)
    for hw, bs in groups.items():
        for b, im in zip(bs, read_batch_u8([images[b] for b in bs], hw, ctx=ctx)):
            out[b] = im
    return out


def save_png(path, rgb):
    """One uint8 (H, W, 3) or (H, W) array as a PNG (PIL; the encoding stays on the host)."""
    from PIL import Image

    Image.fromarray(np.ascontiguousarray(rgb, dtype=np.uint8)).save(path)


def save_pair(out_dir, name, colour, overlay):
    """`<name>.png` and `<name>_overlay.png` under out_dir, as every should_saveimg branch of 03c_hsn and 02_cues names them."""
    os.makedirs(out_dir, exist_ok=True)
    save_png(os.path.join(out_dir, name + ".png"), colour)
    save_png(os.path.join(out_dir, name + "_overlay.png"), overlay)


def quarter_size(shape):
    """The DeepGlobe branches' `dsize=(shape[0] // 4, shape[1] // 4)` (03c_hsn/demo.py:226-227, 02_cues/demo.py:472-473,
    03a_sec-dsrg/model.py:597-600), restated literally: cv2's dsize is (width, height), so the WIDTH comes from the height and
    the height from the width -- moot on DeepGlobe's square images.  Returns (height, width)."""
    return (int(shape[1]) // 4, int(shape[0]) // 4)
