"""float64 restatements of the three kernels that keep the SEC / DSRG prediction loop on the device (csrc/seg_chain.hip), used by
tests/test_seg_chain_oracle.py and tests/test_gpu_seg_chain.py.

    astype_u8     `image.astype(np.uint8)` as include/wsscam.h defines it: truncation toward zero to int32, the low 8 bits
    preprocess    image_preprocess of the evaluation phases (model.py:332-346): TF resize of float(u8), RGB -> BGR, minus the mean
    crf_image     the CRF layer's zoomed image (DSRG.py:318-319,325): x + mean (one fp32 rounding), TF resize, astype_u8
    crf_logprob   the tail of the `crf` closure (DSRG.py:329-332): clamp, sum, divide, log
The TF sampler is tests/deeplab_ref.py's (source coordinates in float32, interpolation in float64)."""
import numpy as np

from tests import deeplab_ref


def astype_u8(v):
    return np.trunc(np.asarray(v, dtype=np.float64)).astype(np.int64).astype(np.int32).astype(np.uint8)


def preprocess(img, mean_bgr, size):
    """img (h, w, 3) uint8 RGB -> (H, W, 3) float64: BGR minus mean_bgr at `size`."""
    r = deeplab_ref.resize_bilinear_tf(np.asarray(img, dtype=np.float64)[None], int(size[0]), int(size[1]))[0]
    return r[:, :, ::-1] - np.asarray(mean_bgr, dtype=np.float32).astype(np.float64).reshape(1, 1, 3)


def crf_image(x, mean, size):
    """x (B, H, W, 3) float32 -> uint8 (B, sh, sw, 3)"""
    v = np.asarray(x, dtype=np.float32) + np.asarray(mean, dtype=np.float32).reshape(1, 1, 1, 3)  # fp32, as the kernel adds it
    return astype_u8(deeplab_ref.resize_bilinear_tf(v, int(size[0]), int(size[1])))


def crf_logprob(q, min_prob):
    """q (B, C, n) class-major marginals -> (B, n, C) float64 log-probabilities"""
    p = np.asarray(q, dtype=np.float64).copy()
    p[p < np.float64(np.float32(min_prob))] = np.float64(np.float32(min_prob))
    p = p / p.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(np.transpose(np.log(p), (0, 2, 1)))
