"""float64 oracle of the SEC / DSRG DeepLab-VGG16 forward pass (03a_sec-dsrg SEC.py:117-128,150-249, DSRG.py:169-300), on torch CPU.

Written from the rules of TensorFlow 1.x the reference's graph relies on, not from TensorFlow (which the test image does not
have: parity with TF itself is unpinned):
  conv            F.conv2d(..., dilation=), padding SAME = dil (k - 1) / 2 for an odd kernel at stride 1
  max pool        explicit F.pad with -inf, pad_before = floor(pad_total / 2)
  average pool    sum over the zero-padded window divided by the pooled ones-mask (the in-image tap count)
  resize          tf.image.resize_bilinear(align_corners=False): src = dst * (in / out), coordinates in float32
  fc8-softmax     e / sum(e) + min_prob, renormalised
Activations are NHWC numpy arrays at the interface, as the reference's tensors are."""
import numpy as np
import torch
import torch.nn.functional as F

TRUNK = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
         "conv5_1", "conv5_2", "conv5_3")
ASPP_RATES = (6, 12, 18, 24)
LFOV_RATE = 12


def same_pad(n, stride, k=3):
    """TF SAME of one axis -> (out, pad_before, pad_after)."""
    out = -(-n // stride)
    total = max((out - 1) * stride + k - n, 0)
    return out, total // 2, total - total // 2


def _nchw(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _pad_same(t, stride, value):
    _, pt, pb = same_pad(t.shape[2], stride)
    _, pl, pr = same_pad(t.shape[3], stride)
    return F.pad(t, (pl, pr, pt, pb), value=value)


def max_pool_same_t(t, stride):
    return F.max_pool2d(_pad_same(t, stride, float("-inf")), 3, stride)


def avg_pool_same_t(t):
    s = F.avg_pool2d(_pad_same(t, 1, 0.0), 3, 1) * 9.0
    n = F.avg_pool2d(_pad_same(torch.ones_like(t[:1, :1]), 1, 0.0), 3, 1) * 9.0
    return s / torch.round(n)


def max_pool_same(x, stride, dtype=torch.float64):
    return _nhwc(max_pool_same_t(_nchw(x, dtype), stride))


def avg_pool_same(x, dtype=torch.float64):
    return _nhwc(avg_pool_same_t(_nchw(x, dtype)))


def conv_t(t, w_hwio, b, dil=1, relu=True):
    w = torch.as_tensor(np.ascontiguousarray(w_hwio)).to(t.dtype).permute(3, 2, 0, 1)
    k = w.shape[2]
    y = F.conv2d(t, w, None if b is None else torch.as_tensor(np.ascontiguousarray(b)).to(t.dtype), stride=1, padding=dil * (k - 1) // 2,
                 dilation=dil)
    return F.relu(y) if relu else y


def resize_bilinear_tf(x, H, W, dtype=np.float64):
    """NHWC; the source coordinates in float32 as TF computes them, the interpolation in `dtype`."""
    x = np.asarray(x, dtype=dtype)
    _, h, w, _ = x.shape

    def axis(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        src = np.arange(n_out, dtype=np.float32) * scale
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, (src - i0.astype(np.float32)).astype(dtype)

    y0, y1, ty = axis(h, H)
    x0, x1, tx = axis(w, W)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    top = x[:, y0][:, :, x0] + (x[:, y0][:, :, x1] - x[:, y0][:, :, x0]) * tx
    bot = x[:, y1][:, :, x0] + (x[:, y1][:, :, x1] - x[:, y1][:, :, x0]) * tx
    return top + (bot - top) * ty


def fc8_softmax(x, min_prob, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True) + dtype(min_prob)
    return p / p.sum(axis=-1, keepdims=True)


def layer_names(method):
    if method == "SEC":
        return TRUNK + ("fc6", "fc7", "fc8")
    if method == "DSRG":
        return TRUNK + tuple("fc%d_%d" % (l, k) for k in (1, 2, 3, 4) for l in (6, 7, 8))
    raise ValueError("method %r" % (method,))


def layer_weights(method, weights):
    """{layer: (w HWIO, b)} from {layer: {'w', 'b'}}; raises on a missing layer or a weight that is not HWIO for its position."""
    out = {}
    cin = 3
    for layer in layer_names(method):
        if layer not in weights:
            raise KeyError("no weights for layer %r" % layer)
        w, b = np.asarray(weights[layer]["w"]), np.asarray(weights[layer]["b"]).reshape(-1)
        k = 3 if (layer.startswith("conv") or layer.startswith("fc6")) else 1
        if layer.startswith("fc6"):
            cin = out["conv5_3"][0].shape[3]
        if w.ndim != 4 or w.shape[0] != k or w.shape[1] != k or w.shape[2] != cin or b.shape[0] != w.shape[3]:
            raise ValueError("layer %r: weights %r are not HWIO [%d][%d][%d][Cout] with a bias of Cout entries" % (layer, w.shape, k, k, cin))
        out[layer] = (w, b)
        cin = w.shape[3]
    return out


def forward(method, weights, x, min_prob=1e-4, dtype=torch.float64):
    """x (B, H, W, 3) -> (fc8 logits, fc8-softmax), both (B, h, w, C) numpy arrays of `dtype`."""
    lw = layer_weights(method, weights)
    t = _nchw(x, dtype)
    for layer in TRUNK:
        t = conv_t(t, lw[layer][0], lw[layer][1], dil=2 if layer.startswith("conv5") else 1)
        if layer in ("conv1_2", "conv2_2", "conv3_3"):
            t = max_pool_same_t(t, 2)
        elif layer in ("conv4_3", "conv5_3"):
            t = max_pool_same_t(t, 1)
    t = avg_pool_same_t(t)

    def branch(sfx, rate):
        u = conv_t(t, *lw["fc6" + sfx], dil=rate)
        u = conv_t(u, *lw["fc7" + sfx])
        return conv_t(u, *lw["fc8" + sfx], relu=False)

    if method == "SEC":
        fc8 = branch("", LFOV_RATE)
    else:
        fc8 = None
        for k, rate in enumerate(ASPP_RATES):
            y = branch("_%d" % (k + 1), rate)
            fc8 = y if fc8 is None else fc8 + y
    fc8 = _nhwc(fc8)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    return fc8, fc8_softmax(fc8, min_prob, np_dtype)


def random_weights(method, num_classes, width=64, fc_width=128, seed=0, widths=None, fc8_gain=0.02):
    """He-scaled random weights {layer: {'w', 'b'}} (activations neither vanish nor saturate); widths: per-trunk-block channel
    counts (5 entries) in place of the one `width`.  The He scale carries the input's magnitude (~100) to fc7; fc8_gain brings
    the logits to the order a trained checkpoint has (|fc8| of a few units up to ~20: its softmax is neither uniform nor a
    one-hot row everywhere), which is what makes a softmax comparison mean something."""
    rng = np.random.default_rng(seed)
    widths = list(widths) if widths is not None else [width] * 5
    out = {}
    cin = 3
    for layer in layer_names(method):
        if layer.startswith("conv"):
            k, cout = 3, widths[int(layer[4]) - 1]
        elif layer.startswith("fc6"):
            k, cout, cin = 3, fc_width, widths[4]
        elif layer.startswith("fc7"):
            k, cout = 1, fc_width
        else:
            k, cout = 1, num_classes
        std = np.sqrt(2.0 / (k * k * cin)) * (fc8_gain if layer.startswith("fc8") else 1.0)
        out[layer] = {"w": (rng.standard_normal((k, k, cin, cout)) * std).astype(np.float32),
                      "b": (rng.standard_normal(cout) * 0.1).astype(np.float32)}
        cin = cout
    return out


# ---- the cases tests/test_gpu_deeplab.py runs end to end, and tests/test_deeplab_oracle.py checks the oracle's own float32 on ----
# (method, classes, (H, W)): 65 x 65 gives 9 x 9 maps, where rates 12 / 18 / 24 are pure centre-tap; 64 x 48 is even and non-square
THIN_CASES = [(m, c, hw) for m in ("SEC", "DSRG") for c in (5, 21) for hw in ((65, 65), (64, 48))]
ARGMAX_AGREE = 0.995


def net_input(B, H, W, seed):
    """BGR minus mean as the reference feeds it: un-normalised, magnitude up to ~150."""
    return np.random.default_rng(seed).uniform(-125.0, 150.0, (B, H, W, 3)).astype(np.float32)


def thin_case(method, C, hw):
    """-> (weights, x) of a thin net (every width 64, fc width 128), B = 2"""
    seed = 100 + 7 * C + hw[1] + (1 if method == "SEC" else 0)
    return random_weights(method, C, 64, 128, seed=seed), net_input(2, hw[0], hw[1], seed + 1)
