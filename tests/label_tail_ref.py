"""float64 references of the kernels that turn maps into LABELS (tests/test_gpu_label_tail.py holds the HIP kernels to them;
tests/test_label_tail_oracle.py holds THEM to torch.double and to hand-written examples).  Plain numpy, one function per entry
point of include/wsscam.h, each restating the reference lines that header cites.  Nothing here touches the device, the
library or the product's own numpy mirrors."""
import numpy as np


def _taps(n_in, n_out):
    """Source taps of F.interpolate(mode='bilinear', align_corners=False) along one axis: (i0, i1, l0, l1)."""
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1


def upsample_bilinear(x, size):
    """F.interpolate(x[None], size, mode='bilinear', align_corners=False)[0] for x [K][h][w], in float64 (make_cam.py:64-69,
    make_sem_seg_labels.py:73 / :91 / :110; sizes below the source's are sampled by the same rule, :102-104)."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 3
    y0, y1, ly0, ly1 = _taps(x.shape[1], int(size[0]))
    x0, x1, lx0, lx1 = _taps(x.shape[2], int(size[1]))
    top = x[:, y0][:, :, x0] * lx0 + x[:, y0][:, :, x1] * lx1
    bot = x[:, y1][:, :, x0] * lx0 + x[:, y1][:, :, x1] * lx1
    return top * ly0[None, :, None] + bot * ly1[None, :, None]


def sem_seg_finish(rw, up_hw, out_hw, keys, has_bg, bg_thres):
    """The tail of make_sem_seg_labels._work for one image (03b_irn/step/make_sem_seg_labels.py:73-79 voc12, :91-96 ADP,
    :110-115 DeepGlobe):
        rw_up = F.interpolate(rw, size=up_hw, 'bilinear', align_corners=False)[..., :H0, :W0]
        rw_up = rw_up / torch.max(rw_up)                    one maximum over all maps and CROPPED pixels
        has_bg: rw_up = F.pad(rw_up, (0, 0, 0, 0, 1, 0), value=bg_thres)
        label = keys[torch.argmax(rw_up, dim=0)]            the first maximum; a NaN counts as the maximum, the first of them wins
    A zero maximum makes every map NaN, so every pixel gets keys[1] (has_bg) or keys[0].
    rw [K][h][w] -> (labels uint8 [H0][W0], the float64 stack [K (+ 1)][H0][W0] the arg-max ran over)."""
    H0, W0 = int(out_hw[0]), int(out_hw[1])
    up = upsample_bilinear(rw, up_hw)[:, :H0, :W0]
    with np.errstate(invalid="ignore", divide="ignore"):
        stack = up / up.max()
    if has_bg:
        stack = np.concatenate([np.full((1, H0, W0), float(bg_thres), np.float64), stack], axis=0)
    keys = np.asarray(keys, dtype=np.int64)
    assert keys.shape == (stack.shape[0],)
    return keys[np.argmax(stack, axis=0)].astype(np.uint8), stack  # np.argmax has torch.argmax's rule: first maximum, first NaN


def top_two_margin(stack):
    """Per pixel, the distance between the largest and the second largest entry of a [M][...] stack (inf for M = 1 and where
    the stack is NaN: there the label follows from a rule, not from arithmetic)."""
    if stack.shape[0] == 1 or np.isnan(stack).any():
        return np.full(stack.shape[1:], np.inf)
    srt = np.sort(stack, axis=0)
    return srt[-1] - srt[-2]


def label_unary_from_cam(maps, thres, gt_prob):
    """cam_to_ir_label's confident-label arg-max (03b_irn/step/cam_to_ir_label.py:33-34 ADP, :45-46 / :50-51 voc12, :64-66
    DeepGlobe) and the energy imutils.crf_inference_label builds from it:
        labels = np.argmax(np.pad(maps, ((1, 0), (0, 0)), constant_values=thres), axis=0)    (maps float32: so is the pad)
        pydensecrf.utils.unary_from_labels(labels, n_labels = K + 1, gt_prob, zero_unsure=False):
            U = full((n_labels, N), -log((1 - gt_prob) / (n_labels - 1)), float32);  U[labels, arange(N)] = -log(gt_prob)
    The ABI takes gt_prob as a float: the energies are those of float64(float32(gt_prob)).
    maps float32 [K][N] -> (labels int32 [N], unary float32 [K + 1][N])."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 2
    K, N = maps.shape
    labels = np.argmax(np.pad(maps, ((1, 0), (0, 0)), mode="constant", constant_values=thres), axis=0)
    g = np.float64(np.float32(gt_prob))
    U = np.full((K + 1, N), -np.log((1.0 - g) / K), dtype=np.float32)
    U[labels, np.arange(N)] = -np.log(g)
    return labels.astype(np.int32), U


def ir_label_combine(fg, bg, keys):
    """cam_to_ir_label's merge for one image (03b_irn/step/cam_to_ir_label.py): fg / bg are the CRF's arg-max over
    [threshold | maps], keys the image's lookup table (voc12: np.pad(keys + 1, (1, 0)); ADP / DeepGlobe: [-1 | keys]).
        voc12 :48, :53, :56-58     conf = keys[fg];  conf[keys[fg] == 0] = 255;  conf[keys[bg] + keys[fg] == 0] = 0
        bg is None :36, :39-40 / :68, :71-72     conf = keys[fg];  conf[conf == -1] = 255
    and the uint8 the PNG holds (:76-77).  fg / bg int [N] -> uint8 [N]."""
    keys = np.asarray(keys, dtype=np.int64)
    fg_conf = keys[np.asarray(fg, dtype=np.int64)]
    conf = fg_conf.copy()
    if bg is not None:
        bg_conf = keys[np.asarray(bg, dtype=np.int64)]
        conf[fg_conf == 0] = 255
        conf[bg_conf + fg_conf == 0] = 0
    else:
        conf[fg_conf == -1] = 255
    return conf.astype(np.uint8)


def cam_sum_scales(cam, n_scales):
    """torch.sum(torch.stack([...per-scale maps...]), 0) of 03b_irn/step/make_cam.py:62-69 in the order the entry point
    documents: image b's n_scales consecutive maps added one after the other in float32.  cam float32 [n_images * n_scales][E]
    -> float32 [n_images][E]; the kernel's result has these bits."""
    cam = np.asarray(cam)
    assert cam.dtype == np.float32 and cam.ndim == 2 and cam.shape[0] % n_scales == 0
    acc = cam[0::n_scales].copy()
    for s in range(1, n_scales):
        acc = acc + cam[s::n_scales]  # float32 + float32: one rounding per scale
    return acc


def hsn_voc_background(Hbg):
    """03c_hsn/demo.py:146-147: X_bg = np.sum(H['bg'], axis=1); Y[:, 0] = 0.15 * scipy.special.expit(np.max(X_bg) - X_bg),
    the maximum over the WHOLE batch.  Hbg [B][Cb][N] -> float64 [B][N].  (expit(z) = 1 / (1 + exp(-z)); z >= 0 here.)"""
    X = np.asarray(Hbg, dtype=np.float64).sum(axis=1)
    return 0.15 / (1.0 + np.exp(-(X.max() - X)))


def class_mass(maps):
    """dcrf_process keeps the classes whose map has mass (03c_hsn/utilities.py:425): maps [n][N] -> bool [n]."""
    return np.asarray(maps, dtype=np.float64).sum(axis=-1) > 0
