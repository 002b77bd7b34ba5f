"""float64 references of the small network-internal layers (tests/test_gpu_layers.py holds the HIP kernels to them; tests/
test_layer_ref_host.py holds THEM to torch.nn / hand-written loops).  Plain numpy / torch.double, nothing here touches the
device or the library."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import bf16_round, f16_round
from wsscam import _lib

TWO_PLANE = (_lib.PREC_BF16X3, _lib.PREC_F16X3)
ALL_PRECISIONS = (_lib.PREC_BF16, _lib.PREC_BF16X3, _lib.PREC_F16, _lib.PREC_F16X3, _lib.PREC_F32)
PREC_NAME = {_lib.PREC_BF16: "bf16", _lib.PREC_BF16X3: "bf16x3", _lib.PREC_F16: "f16", _lib.PREC_F16X3: "f16x3", _lib.PREC_F32: "f32"}
# the half-ulp of a value the activation planes of a precision hold, relative (two planes: 8 + 8 / 11 + 11 significand bits)
HALF_ULP = {_lib.PREC_BF16: 2.0 ** -8, _lib.PREC_F16: 2.0 ** -11, _lib.PREC_BF16X3: 2.0 ** -16, _lib.PREC_F16X3: 2.0 ** -22,
            _lib.PREC_F32: 0.0}
# IEEE half is subnormal below 2^-14 (spacing 2^-24): an absolute half-spacing on top of the relative one
ABS_FLOOR = {_lib.PREC_BF16: 0.0, _lib.PREC_BF16X3: 0.0, _lib.PREC_F16: 2.0 ** -25, _lib.PREC_F16X3: 2.0 ** -25, _lib.PREC_F32: 0.0}


def round16(x, prec):
    """x (float32) rounded to the 16-bit format of the precision's planes, as float32."""
    return bf16_round(x) if prec in (_lib.PREC_BF16, _lib.PREC_BF16X3) else f16_round(x)


def planes(x, prec):
    """(hi, lo) float32 planes of a 16-bit precision for float32 x; lo is None in the one-plane modes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = round16(x, prec)
    return hi, (round16(x - hi, prec) if prec in TWO_PLANE else None)


def as_precision(x, prec):
    """The value the activation planes of `prec` hold for a float32 x, as float32: round16(x) in the one-plane modes, hi + lo
    with lo = round16(x - hi) in the two-plane modes (x - hi is exact; hi + lo is exact in fp32, both planes lying inside
    x's 24-bit window), x itself in PREC_F32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if prec == _lib.PREC_F32:
        return x.copy()
    hi, lo = planes(x, prec)
    return hi if lo is None else hi + lo


def group_stats(x, G, eps):
    """Per (sample, group) of NHWC x: (mean, rstd, max|x|) in float64, two-pass, biased variance, eps inside the root."""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, C = x.shape
    g = x.reshape(N, H * W, G, C // G).transpose(0, 2, 1, 3).reshape(N, G, -1)
    mean = g.mean(-1)
    var = ((g - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / np.sqrt(var + float(eps)), np.abs(g).max(-1)


def group_norm_head(x, gamma, beta, G, eps, up, relu, Hd, Wd, y_init, coff):
    """One IRNet head after its convolution in the nets' own order: F.group_norm (double), nn.Upsample(scale_factor = up,
    'bilinear', align_corners = False), crop [:Hd, :Wd], ReLU, written to channels [coff, coff + C) of a copy of y_init
    (N, Hd, Wd, Ctot).  x NHWC (N, H, W, C).  Returns float64 (N, Hd, Wd, Ctot)."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    C = xt.shape[1]
    y = F.group_norm(xt, G, torch.from_numpy(np.asarray(gamma, dtype=np.float64)), torch.from_numpy(np.asarray(beta, dtype=np.float64)),
                     float(eps))
    if up != 1:
        y = F.interpolate(y, scale_factor=up, mode="bilinear", align_corners=False)
    y = y[:, :, :Hd, :Wd]
    if relu:
        y = torch.relu(y)
    out = np.array(y_init, dtype=np.float64)
    assert out.shape[:3] == (xt.shape[0], Hd, Wd) and coff + C <= out.shape[3]
    out[..., coff:coff + C] = y.permute(0, 2, 3, 1).numpy()
    return out


def max_pool(x, k, stride, pad):
    """nn.MaxPool2d(k, stride, pad) of NHWC x in float64 (F.max_pool2d pads with -inf)."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    return np.ascontiguousarray(F.max_pool2d(xt, k, stride, pad).permute(0, 2, 3, 1).numpy())


def gap(feat, use_max, sample_stride):
    """feat (n_samples, npix, F) -> the pooled (B, F) features of samples 0, stride, 2 stride, ... in float64."""
    f = np.asarray(feat, dtype=np.float64)[::sample_stride]
    return f.max(1) if use_max else f.mean(1)


def gap_linear_sigmoid(feat, w, bias, use_max, sample_stride):
    """sigmoid(bias + W . pool(feat[stride b])) in float64 -> (score (B, C), pooled (B, F))."""
    g = gap(feat, use_max, sample_stride)
    z = g @ np.asarray(w, dtype=np.float64).T
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-z)), g


def flip_add(head, C):
    """head (2B, h, w, Cs) float32 NHWC -> cam (B, C, h, w) = relu(head[2b]) + relu(head[2b + 1]).flip(w), in head's dtype."""
    r = np.maximum(head[..., :C], 0)
    return np.ascontiguousarray((r[0::2] + r[1::2, :, ::-1]).transpose(0, 3, 1, 2))


def edge_finish(e, d, fh, fw, ms):
    """e (2B, He, We), d (2B, Hd, Wd, 2) float32 -> (edge (B, fh, fw) float64 = sigmoid(e[2b] / 2 + flip(e[2b + 1][:fh, :fw]) / 2),
    dp (B, 2, fh, fw) = d[2b][:fh, :fw] - ms in d's dtype): crop, THEN flip."""
    ec = np.asarray(e, dtype=np.float64)[:, :fh, :fw]
    z = ec[0::2] / 2 + ec[1::2, :, ::-1] / 2
    dp = d[0::2, :fh, :fw, :] - np.asarray(ms, dtype=d.dtype)
    return 1.0 / (1.0 + np.exp(-z)), np.ascontiguousarray(dp.transpose(0, 3, 1, 2))
