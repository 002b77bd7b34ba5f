"""VOC12 MSF classification dataset -- input contract of make_cam
(03b_irn/voc12/dataloader.py: load_img_name_list :60-66, TorchvisionResize :68-78,
TorchvisionNormalize :80-106, VOC12ClassificationDatasetMSF :210-246).

Items are dicts {"name", "img": float32 (2,3,S,S) [orig, h-flip], "size": (H0,W0), "label"}.
JPEG decode uses PIL (imageio/cv2 are not in this image).  The float64 bilinear resize follows
cv2.resize's INTER_LINEAR half-pixel convention; cv2 itself is absent offline so bit parity of
this host-side resize is unpinned -- it is I/O, outside the device hot path."""
import os

import numpy as np

IMG_FOLDER_NAME = "JPEGImages"


def decode_int_filename(int_filename):
    s = str(int(int_filename))
    return s[:4] + "_" + s[4:]


def load_img_name_list(dataset_path):
    names = [l.strip() for l in open(dataset_path) if l.strip()]
    return np.array([np.int32(int(n.split("_")[0]) * 1e6 + int(n.split("_")[1])) for n in names])


def get_img_path(img_name, voc12_root):
    if not isinstance(img_name, str):
        img_name = decode_int_filename(img_name)
    return os.path.join(voc12_root, IMG_FOLDER_NAME, img_name + ".jpg")


def resize_bilinear_f64(img, out_hw):
    H, W = img.shape[:2]
    oh, ow = int(out_hw[0]), int(out_hw[1])
    im = np.asarray(img, dtype=np.float64)
    if (H, W) == (oh, ow):
        return im
    ys = np.clip((np.arange(oh) + 0.5) * H / oh - 0.5, 0, H - 1)
    xs = np.clip((np.arange(ow) + 0.5) * W / ow - 0.5, 0, W - 1)
    y0 = np.floor(ys).astype(int)
    x0 = np.floor(xs).astype(int)
    y1 = np.minimum(y0 + 1, H - 1)
    x1 = np.minimum(x0 + 1, W - 1)
    wy = (ys - y0)[:, None, None]
    wx = (xs - x0)[None, :, None]
    top = im[y0][:, x0] * (1 - wx) + im[y0][:, x1] * wx
    bot = im[y1][:, x0] * (1 - wx) + im[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def _cv2_linear_taps_u8(src, dst, clamp_taps):
    """Source index and the two 11-bit fixed-point coefficients of OpenCV's 8-bit INTER_LINEAR along one axis."""
    scale = 1.0 / (np.float64(dst) / np.float64(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if clamp_taps:  # columns: the window is moved inside and the fraction dropped
        lo, hi = s < 0, s >= src - 1
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        f = np.where(lo | hi, np.float32(0), f)
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)  # saturate_cast<short>: round half to even
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, c0, c1


def resize_bilinear_u8(img, out_hw):
    """cv2.resize(uint8 image, (w, h)) with the default INTER_LINEAR, as read_batch of 02_cues/utilities.py:172-176 and
    03c_hsn/utilities.py:176-181 get it (the batch array is uint8).  OpenCV's 8-bit path is fixed point -- 11-bit
    coefficients, an int horizontal pass, the vertical pass (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2 --
    and an exact 2 x 2 decimation is the rounded box mean (INTER_AREA shortcut); restated from the published algorithm
    (cv2 is absent offline: parity against cv2 itself unpinned).  Bit-identical to wsc_resize_u8 (csrc/input.hip)."""
    im = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = im.shape[:2]
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if (H, W) == (oh, ow):
        return im.copy()
    v = im.astype(np.int64)
    if (H, W) == (2 * oh, 2 * ow):
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _cv2_linear_taps_u8(W, ow, True)
    sy, b0, b1 = _cv2_linear_taps_u8(H, oh, False)
    x1 = np.minimum(sx + 1, W - 1)
    y0, y1 = np.clip(sy, 0, H - 1), np.clip(sy + 1, 0, H - 1)
    hor = v[:, sx] * a0[None, :, None] + v[:, x1] * a1[None, :, None]  # (H, ow, 3) int
    out = (((b0[:, None, None] * (hor[y0] >> 4)) >> 16) + ((b1[:, None, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


class TorchvisionNormalize:
    def __init__(self, norm_mode="int"):
        self.norm_mode = norm_mode
        if norm_mode == "int":
            self.mean, self.std = (104.0, 117.0, 123.0), (255.0, 255.0, 255.0)
        elif norm_mode == "float":
            self.mean, self.std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        elif norm_mode is not None:
            raise ValueError("norm_mode value is not 'int' or 'float'")

    def __call__(self, img):
        proc = np.empty(img.shape, np.float32)
        img = np.float32(img)
        for c in range(3):
            if self.norm_mode == "int":
                proc[..., c] = (img[..., c] - self.mean[c]) / self.std[c]
            elif self.norm_mode == "float":
                proc[..., c] = (img[..., c] / 255.0 - self.mean[c]) / self.std[c]
            else:
                return img
        return proc


def msf_pack(img_u8, outsize, norm):
    x = norm(resize_bilinear_f64(img_u8, outsize) if outsize is not None else np.asarray(img_u8, np.float64))
    x = np.transpose(x, (2, 0, 1))
    return np.stack([x, np.flip(x, -1)], axis=0).astype(np.float32)


class VOC12ClassificationDatasetMSF:
    def __init__(self, img_name_list_path, dev_root, norm_mode="float", outsize=None, scales=(1.0,),
                 cls_labels_path=None, device_transform=False):
        assert norm_mode in ["float", "int"]
        assert outsize in [(321, 321), (224, 224), None]
        self.scales = tuple(scales)
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.dev_root = dev_root
        self.outsize = outsize
        self.norm = TorchvisionNormalize(norm_mode)
        # device_transform: items carry the decoded image ("img_u8") instead of the float32 pair ("img"); make_cam's
        # pipeline then runs resize + normalise + flip on the GPU (wsc_msf_input_u8, bit-identical to msf_pack)
        self.device_transform = device_transform and outsize is not None
        from ..adp.dataloader import find_cls_labels

        cls = np.load(find_cls_labels(os.path.join("voc12", "cls_labels.npy"), cls_labels_path),
                      allow_pickle=True).item()
        self.label_list = np.array([cls[n] for n in self.img_name_list])

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        from PIL import Image

        name_str = decode_int_filename(self.img_name_list[idx])
        img = np.asarray(Image.open(get_img_path(name_str, self.dev_root)).convert("RGB"))
        # voc12/dataloader.py:231-242: every scale is rescaled (PIL bicubic), then resized to `outsize` like the plain image;
        # one scale -> the array itself, several -> a list (the reference's item format)
        from ..misc import imutils

        s_imgs = imutils.scale_images(img, self.scales)
        if self.device_transform:
            return {"name": name_str, "img_u8": s_imgs[0] if len(s_imgs) == 1 else s_imgs, "size": (img.shape[0], img.shape[1]),
                    "label": self.label_list[idx]}
        ms = [msf_pack(si, self.outsize, self.norm) for si in s_imgs]
        return {"name": name_str, "img": ms[0] if len(ms) == 1 else ms, "size": (img.shape[0], img.shape[1]),
                "label": self.label_list[idx]}


class VOC12ImageDataset:
    """voc12/dataloader.py:137-190 as cam_to_ir_label uses it (`norm_mode=None, to_torch=False`, cam_to_ir_label.py:100-101):
    items {"name", "img": uint8 HWC}.  The training-time augmentations of the class (resize_long, rescale, crops, flips)
    belong to train_cam / train_irn, which are out of scope."""

    def __init__(self, img_name_list_path, dev_root, norm_mode=None, to_torch=False, **augment):
        if any(v for v in augment.values()) or norm_mode is not None or to_torch:
            raise NotImplementedError("VOC12ImageDataset: only the plain image reader of the inference steps is provided")
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.dev_root = dev_root

    def __len__(self):
        return len(self.img_name_list)

    def __getitem__(self, idx):
        from PIL import Image

        name_str = decode_int_filename(self.img_name_list[idx])
        return {"name": name_str, "img": np.asarray(Image.open(get_img_path(name_str, self.dev_root)).convert("RGB"))}


class SegmentationDatasetBase:
    """The sample transform the three *SegmentationDataset classes of the reference share (voc12/dataloader.py:248-300,
    adp/dataloader.py:242-300, deepglobe/dataloader.py:233-287), split so that the device can apply the same random choices:

        decoded(idx)        -> (uint8 (H, W, 3) image, uint8 (H, W) label): the two files, decoded (PIL)
        draw(idx, hw=None)  -> the parameter record, int32 (9,) in the order of _lib.IRN_BATCH_PARAMS: (scaled_h, scaled_w,
                               flip, cont_top, cont_left, img_top, img_left, ch, cw).  The draws are the reference's, from
                               Python's `random` in its order: random.random() (rescale), random.getrandbits(1) (hor_flip),
                               imutils.get_random_crop_box's two randrange (crop_method 'random').  hw: the image's size where
                               the caller has it (else the file's header is read)
        item(idx, params, decoded=None)   the record applied on the host -> {'name', 'img' float32 (3, S, S), 'label' uint8
                               (S, S)}: rescale (PIL bicubic / nearest) or TorchvisionResize (image AND label), normalise,
                               flip, crop into the 0.0 / 255 containers, HWC -> CHW.  The reference's label is float64 from
                               TorchvisionResize on; its only reader is imutils.pil_resize, which takes np.uint8 of it first, so
                               the label is truncated here
        __getitem__(idx)    item(idx, draw(idx))

    irn_train.TrainBatcher.apply(images, labels, params) computes the same arrays on the device (wsc_irn_train_batch), to the bit.
    Subclasses give `names`, image_path(name), the label file's stem and their TorchvisionNormalize."""
    normalize_cls = TorchvisionNormalize

    def __init__(self, label_dir, crop_size, outsize=None, rescale=None, norm_mode="int", hor_flip=False, crop_method="random"):
        if rescale and outsize is not None:
            raise ValueError("rescale together with outsize: no reference configuration combines them")
        if norm_mode not in ("int", "float"):
            raise ValueError("norm_mode value is not 'int' or 'float'")
        self.label_dir = label_dir
        self.crop_size = int(crop_size)
        self.outsize = None if outsize is None else (int(outsize[0]), int(outsize[1]))
        self.rescale = tuple(rescale) if rescale else None
        self.norm_mode = norm_mode
        self.img_normal = self.normalize_cls(norm_mode)
        self.hor_flip = hor_flip
        self.crop_method = crop_method

    def __len__(self):
        return len(self.img_name_list)

    def name_str(self, idx):
        return str(self.img_name_list[idx])

    def image_path(self, name_str):
        raise NotImplementedError

    def decoded(self, idx):
        from PIL import Image

        name_str = self.name_str(idx)
        img = np.asarray(Image.open(self.image_path(name_str)).convert("RGB"))
        label = np.asarray(Image.open(os.path.join(self.label_dir, name_str + ".png")))
        if label.ndim != 2 or label.dtype != np.uint8 or label.shape != img.shape[:2]:
            raise ValueError("label %s.png is %r %s, expected uint8 %r" % (name_str, label.shape, label.dtype, img.shape[:2]))
        return img, label

    def draw(self, idx, hw=None):
        import random

        from ..misc import imutils

        if hw is None:
            from PIL import Image

            with Image.open(self.image_path(self.name_str(idx))) as im:
                hw = (im.size[1], im.size[0])
        sh, sw = int(hw[0]), int(hw[1])
        if self.rescale:  # imutils.random_scale -> pil_rescale's target size
            f = self.rescale[0] + random.random() * (self.rescale[1] - self.rescale[0])
            sh, sw = int(np.round(sh * f)), int(np.round(sw * f))
        if self.outsize is not None:
            sh, sw = self.outsize
        flip = int(bool(random.getrandbits(1))) if self.hor_flip else 0
        S = self.crop_size
        if self.crop_method == "random":
            b = imutils.get_random_crop_box((sh, sw), S)
            box = (b[0], b[2], b[4], b[6], b[1] - b[0], b[3] - b[2])
        elif self.crop_method is not None:  # imutils.top_left_crop
            box = (0, 0, 0, 0, min(S, sh), min(S, sw))
        else:
            if (sh, sw) != (S, S):
                raise ValueError("crop_method None on a %dx%d sample: the batch needs %dx%d" % (sh, sw, S, S))
            box = (0, 0, 0, 0, S, S)
        return np.array((sh, sw, flip) + box, np.int32)

    def item(self, idx, params, decoded=None):
        from ..misc import imutils

        img, label = decoded if decoded is not None else self.decoded(idx)
        sh, sw, flip, cont_top, cont_left, img_top, img_left, ch, cw = (int(v) for v in params)
        if self.outsize is not None:  # TorchvisionResize, image and label (float64)
            img, label = resize_bilinear_f64(img, (sh, sw)), resize_bilinear_f64(label[..., None], (sh, sw))[..., 0]
        else:
            img, label = imutils.pil_resize(img, (sh, sw), 3), imutils.pil_resize(label, (sh, sw), 0)
        img = self.img_normal(img)
        if flip:
            img, label = np.fliplr(img), np.fliplr(label)
        S = self.crop_size
        x = np.zeros((S, S, 3), np.float32)
        lab = np.full((S, S), 255, label.dtype)
        x[cont_top:cont_top + ch, cont_left:cont_left + cw] = img[img_top:img_top + ch, img_left:img_left + cw]
        lab[cont_top:cont_top + ch, cont_left:cont_left + cw] = label[img_top:img_top + ch, img_left:img_left + cw]
        return {"name": self.img_name_list[idx], "img": np.ascontiguousarray(np.transpose(x, (2, 0, 1))), "label": np.uint8(lab)}

    def __getitem__(self, idx):
        dec = self.decoded(idx)
        return self.item(idx, self.draw(idx, dec[0].shape[:2]), dec)


class AffinityDatasetMixin:
    """*AffinityDataset.__getitem__ (voc12/dataloader.py:314-321): adds 'reduced_label' = imutils.pil_rescale(label, 0.25, 0),
    the array irn_train.AffinityLoss takes.  The three pair-label tensors of GetAffinityLabelFromIndices are what
    wsc_irn_aff_loss computes from it on the device, so they are not materialised (indices_from / indices_to are accepted and
    unused)."""

    def item(self, idx, params, decoded=None):
        from ..misc import imutils

        out = super().item(idx, params, decoded)
        out["reduced_label"] = np.ascontiguousarray(imutils.pil_rescale(out["label"], 0.25, 0))
        return out


class VOC12SegmentationDataset(SegmentationDatasetBase):
    """voc12/dataloader.py:248-300."""

    def __init__(self, img_name_list_path, label_dir, crop_size, dev_root, outsize=None, rescale=None, norm_mode="int",
                 hor_flip=False, crop_method="random"):
        super().__init__(label_dir, crop_size, outsize, rescale, norm_mode, hor_flip, crop_method)
        self.img_name_list = load_img_name_list(img_name_list_path)
        self.dev_root = dev_root

    def name_str(self, idx):
        return decode_int_filename(self.img_name_list[idx])

    def image_path(self, name_str):
        return get_img_path(name_str, self.dev_root)


class VOC12AffinityDataset(AffinityDatasetMixin, VOC12SegmentationDataset):
    """voc12/dataloader.py:302-321."""

    def __init__(self, img_name_list_path, label_dir, crop_size, dev_root, indices_from=None, indices_to=None, rescale=None,
                 norm_mode="int", hor_flip=False, crop_method=None, outsize=None):
        super().__init__(img_name_list_path, label_dir, crop_size, dev_root, outsize, rescale, norm_mode, hor_flip, crop_method)
