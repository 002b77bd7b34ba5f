"""float64 reference of a forward pass ONE OP AT A TIME (tests/test_gpu_net_trace.py holds every op of a traced device run to it;
tests/test_net_trace_host.py holds IT to oracle/cnn_ref.py and tests/deeplab_ref.py).

`resnet50_layers`, `plain_layers` and `deeplab_layers` turn a state dict into the list of ops the library runs for it (csrc/net.hip),
each a `Layer`: the label wsc_net_trace_plan gives the op, the entries that produce its operands, and a closure in torch double
built from the state dict itself -- BatchNorm is folded here, in double, from running_mean / running_var / weight / bias (eps 1e-5
ResNet, 1e-3 the plain stacks), never from the library's fp32 scale / shift.  A conv closure returns

    ref  the op's output,
    A    = conv(|x|, |w|) |scale| + ... + |shift| + |residual|: what every rounding of the op is relative to,
    S    = conv(|x|, 1) max|w_c| |scale|: what an ABSOLUTE error of a weight (a half subnormal) is relative to,

pools and gathers return (ref, None, None).  Operands and results are NCHW torch.float64 tensors.  Nothing here touches the device
or the library."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn_ref
from tests import deeplab_ref, keras_arch_ref, layer_ref
from tests.helpers import f16_round

INPUT, NONE = -1, -2  # producer codes of wsc_trace_op


class Layer:
    def __init__(self, label, kind, fn, inputs, **kw):
        self.label, self.kind, self.fn = label, kind, fn
        self.inputs = inputs            # (in, in2, res): indices into the layer list, INPUT or NONE
        self.K = kw.get("K", 0)         # conv / head: products per output element
        self.steps = kw.get("steps", 0)  # roundings of the epilogue beyond scale + shift (residual add, second affine, sigma fold)
        self.entry = kw.get("entry", False)   # the stage-entry GEMM: weights w s / sigma, rounded once more before the split
        self.concat_with = kw.get("concat_with")  # gather: the entry whose channels come first in the tensor it completes
        self.weights = kw.get("weights", ())  # state-dict keys of the conv weights the op implements
        self.pool = kw.get("pool")      # pool: (rule, k, stride, pad, avg), rule as PoolRule of csrc/common.h


def _d(t):
    return torch.as_tensor(np.asarray(t)).double()


def fold_bn(sd, bn, eps):
    """(scale, shift) of inference BatchNorm in double"""
    s = _d(sd[bn + ".weight"]) / torch.sqrt(_d(sd[bn + ".running_var"]) + eps)
    return s, _d(sd[bn + ".bias"]) - _d(sd[bn + ".running_mean"]) * s


def round_weights_f16(w):
    """OIHW double -> the values WSC_PREC_F16 holds for them: every output channel times the power of two that puts its largest
    |w| into [2^12, 2^13), rounded to IEEE half, scaled back (csrc/net.hip make_conv)"""
    w32 = w.float().numpy()
    mx = np.abs(w32).reshape(w32.shape[0], -1).max(1)
    sh = np.where(mx > 0, 13 - np.frexp(np.where(mx > 0, mx, 1.0))[1], 0).astype(np.int32)
    sc = np.ldexp(np.float32(1), sh)[:, None, None, None]
    return torch.from_numpy(f16_round(w32 * sc).astype(np.float64) / sc.astype(np.float64))


def split_weights_f16x3(w):
    """... and the hi + lo pair WSC_PREC_F16X3 holds (lo = half(w 2^sh - hi)); only the mutant checks feed a reference these"""
    w32 = w.float().numpy()
    mx = np.abs(w32).reshape(w32.shape[0], -1).max(1)
    sh = np.where(mx > 0, 13 - np.frexp(np.where(mx > 0, mx, 1.0))[1], 0).astype(np.int32)
    sc = np.ldexp(np.float32(1), sh)[:, None, None, None]
    hi = f16_round(w32 * sc)
    lo = f16_round(w32 * sc - hi)
    return torch.from_numpy((hi.astype(np.float64) + lo.astype(np.float64)) / sc.astype(np.float64))


def _pc(v):
    return v[None, :, None, None]


def _conv_terms(x, w, stride=1, pad=0, dil=1):
    """(conv(x, w), conv(|x|, |w|), conv(|x|, 1) max_c |w|) of one source"""
    y = F.conv2d(x, w, stride=stride, padding=pad, dilation=dil)
    a = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad, dilation=dil)
    ones = torch.ones(1, 1, w.shape[2], w.shape[3], dtype=torch.float64)
    s = F.conv2d(x.abs().sum(1, keepdim=True), ones, stride=stride, padding=pad, dilation=dil)
    return y, a, s * _pc(w.abs().flatten(1).max(1).values)


def conv_affine(w, scale, shift, stride, pad, relu, dil=1, wround=None):
    """[relu](conv(x, w) scale + shift [+ res])"""
    w = _d(w)
    if wround:
        w = wround(w)

    def fn(x, x2=None, res=None):
        y, a, s = _conv_terms(x, w, stride, pad, dil)
        ref = y * _pc(scale) + _pc(shift)
        A = a * _pc(scale).abs() + _pc(shift).abs()
        if res is not None:
            ref, A = ref + res, A + res.abs()
        return (torch.relu(ref) if relu else ref), A, s * _pc(scale).abs()
    return fn


def stage_entry(w3, s3, b3, wd, sd_, bd, stride, wround=None, mutate=None, sigma="max"):
    """relu(bn3(conv3(y2)) + bn_d(conv_d(x[:, :, ::s, ::s]))) (resnet50.py:44-52).  x2 None: x is the materialised concatenation
    [y2 | x at the stride].  wround: the weights as a one-plane mode holds them -- w s / sigma with sigma = max(|s3|, |sd|), the
    fold of csrc/net.hip, rounded, and sigma kept as the scale.  mutate / sigma = "s3" (sigma = |s3| alone): wrong versions, for the
    mutant checks only."""
    w3, wd = _d(w3), _d(wd)
    K1 = w3.shape[1]
    if wround:
        sig = torch.maximum(s3.abs(), sd_.abs()) if sigma == "max" else s3.abs()
        sig = torch.where(sig > 0, sig, torch.ones_like(sig))
        w3, wd = wround(torch.cat([w3 * (s3 / sig)[:, None, None, None], wd * (sd_ / sig)[:, None, None, None]], 1)).split([K1, wd.shape[1]], 1)
        s3 = sd_ = sig

    def fn(x, x2=None, res=None):
        if x2 is None:
            y2, xs = x[:, :K1], x[:, K1:]
        elif mutate == "tap":  # the second source one row off (clamped)
            idx = torch.clamp(torch.arange(0, x2.shape[2], stride) + 1, max=x2.shape[2] - 1)[:x.shape[2]]
            y2, xs = x, x2[:, :, idx][:, :, :, ::stride]
        else:
            y2, xs = x, x2[:, :, ::stride, ::stride]
        ya, aa, sa = _conv_terms(y2, w3)
        yb, ab, sb = _conv_terms(xs, wd)
        ref = ya * _pc(s3) + yb * _pc(sd_) + _pc(b3 + bd)
        A = aa * _pc(s3).abs() + ab * _pc(sd_).abs() + _pc(b3).abs() + _pc(bd).abs()
        return torch.relu(ref), A, sa * _pc(s3).abs() + sb * _pc(sd_).abs()
    return fn


def plain_conv(w, bias, s2, b2, pad=1, dil=1, wround=None, mutate=None):
    """bn(relu(conv(x) + bias)) of common_cnn.make_layers (s2 None: no BatchNorm)"""
    w, bias = _d(w), _d(bias)
    if wround:
        w = wround(w)

    def fn(x, x2=None, res=None):
        y, a, s = _conv_terms(x, w, 1, pad, dil)
        z, A = y + _pc(bias), a + _pc(bias).abs()
        if s2 is None:
            return torch.relu(z), A, s
        if mutate == "affine_before_relu":
            return torch.relu(z * _pc(s2) + _pc(b2)), A * _pc(s2).abs() + _pc(b2).abs(), s * _pc(s2).abs()
        return torch.relu(z) * _pc(s2) + _pc(b2), A * _pc(s2).abs() + _pc(b2).abs(), s * _pc(s2).abs()
    return fn


POOL_TORCH, POOL_TF_SAME, POOL_TF_VALID = 0, 1, 2


def pool(rule, k, stride, pad, avg):
    """the window loops of tests/layer_ref.py, tests/keras_arch_ref.py and tests/deeplab_ref.py, by the rule of the op"""
    def fn(x, x2=None, res=None):
        nhwc = x.permute(0, 2, 3, 1).contiguous().numpy()
        if avg:
            assert rule == POOL_TF_SAME and k == 3 and stride == 1
            y = deeplab_ref.avg_pool_same(nhwc)
        elif rule == POOL_TORCH:
            y = layer_ref.max_pool(nhwc, k, stride, pad)
        else:
            y = keras_arch_ref.tf_max_pool(nhwc, k, stride, rule == POOL_TF_SAME)
        return torch.from_numpy(np.ascontiguousarray(y)).permute(0, 3, 1, 2), None, None
    return fn


def gather(stride):
    def fn(x, x2=None, res=None):
        return x[:, :, ::stride, ::stride], None, None
    return fn


def head(w, bias=None, wround=None):
    """the 1x1 head before the ReLU and the pair sum: einsum over the feature map"""
    w = _d(w).reshape(w.shape[0], -1)
    if wround:
        w = wround(w[:, :, None, None])[:, :, 0, 0]

    def fn(x, x2=None, res=None):
        ref = torch.einsum("nfhw,cf->nchw", x, w)
        A = torch.einsum("nfhw,cf->nchw", x.abs(), w.abs())
        if bias is not None:
            ref, A = ref + _pc(_d(bias)), A + _pc(_d(bias)).abs()
        return ref, A, x.abs().sum(1, keepdim=True) * _pc(w.abs().max(1).values)
    return fn


def cam_from_head(h):
    """[orig, flip] pair sum of resnet50_cam.py:65-66: (2B, C, h, w) head output -> (B, C, h, w)"""
    r = torch.relu(h)
    return r[0::2] + r[1::2].flip(-1)


# ---- the op lists ----------------------------------------------------------------------------------------------------------------
def resnet50_layers(sd, prec, with_head=True, mutate=None):
    """prec: 'f32' (separate projection + residual), 'f16x3' / 'f16' (two-source stage entry), 'bf16x3' (materialised stage entry)"""
    wround = round_weights_f16 if prec == "f16" else None
    L = []

    def add(*a, **kw):
        L.append(Layer(*a, **kw))
        return len(L) - 1

    def conv_bn(name, bn, stride, pad, relu, src, res=NONE):
        w = sd[name + ".weight"]
        s, b = fold_bn(sd, bn, 1e-5)
        return add(name, "conv", conv_affine(w, s, b, stride, pad, relu, wround=wround), (src, NONE, res),
                   K=int(np.prod(w.shape[1:])), steps=1 if res != NONE else 0, weights=(name + ".weight",))

    cur = conv_bn("resnet50.conv1", "resnet50.bn1", 2, 3, True, INPUT)
    cur = add("pool:0", "pool", pool(POOL_TORCH, 3, 2, 1, False), (cur, NONE, NONE), pool=(POOL_TORCH, 3, 2, 1, 0))
    for li, (blocks, stride) in enumerate(zip(cnn_ref.RESNET_BLOCKS, (1,) + cnn_ref.RESNET_CAM_STRIDES[1:])):
        for bi in range(blocks):
            pre = "resnet50.layer%d.%d" % (li + 1, bi)
            s = stride if bi == 0 else 1
            c1 = conv_bn(pre + ".conv1", pre + ".bn1", 1, 0, True, cur)
            c2 = conv_bn(pre + ".conv2", pre + ".bn2", s, 1, True, c1)
            down = pre + ".downsample.0.weight" in sd
            if down and prec != "f32":
                w3, wd = sd[pre + ".conv3.weight"], sd[pre + ".downsample.0.weight"]
                s3, b3 = fold_bn(sd, pre + ".bn3", 1e-5)
                sd_, bd = fold_bn(sd, pre + ".downsample.1", 1e-5)
                if mutate in ("sigma", "split"):  # the f16x3 weight pairs of the fold with sigma = |s3| alone / of the fold as it is
                    fn = stage_entry(w3, s3, b3, wd, sd_, bd, s, wround=split_weights_f16x3, sigma="s3" if mutate == "sigma" else "max")
                else:
                    fn = stage_entry(w3, s3, b3, wd, sd_, bd, s, wround=wround, mutate=mutate)
                kw = dict(K=w3.shape[1] + wd.shape[1], steps=3, entry=True, weights=(pre + ".conv3.weight", pre + ".downsample.0.weight"))
                if prec == "bf16x3":
                    g = add(pre + ".gather", "gather", gather(s), (cur, NONE, NONE), concat_with=c2)
                    cur = add(pre + ".conv3+downsample", "conv", fn, (g, NONE, NONE), **kw)
                else:
                    cur = add(pre + ".conv3+downsample", "conv", fn, (c2, cur, NONE), **kw)
                continue
            res = cur
            if down:
                res = conv_bn(pre + ".downsample.0", pre + ".downsample.1", s, 0, False, cur)
            cur = conv_bn(pre + ".conv3", pre + ".bn3", 1, 0, True, c2, res)
    if with_head:
        w = sd["classifier.weight"]
        add("head", "head", head(w, wround=wround), (cur, NONE, NONE), K=w.shape[1], weights=("classifier.weight",))
    return L


def plain_layers(sd, root, cfg, pools=None, head_w=None, head_bias=None, prec="f32", mutate=None):
    """common_cnn.make_layers stacks (vgg16 / m7); pools: the (k, stride, same) rows of a `pool_spec`, else MaxPool2d(2, 2);
    head_w (C, F): the 1x1 head's weights (the Linear weight, or the transposed Grad-CAM alpha)"""
    wround = round_weights_f16 if prec == "f16" else None
    L = []
    cur, n_pool = INPUT, 0
    for lname, layer in cfg:
        idx = 0
        for v in layer:
            if v == "M":
                if pools is not None:
                    k, stride, same = [int(t) for t in pools[n_pool]]
                    geom = (POOL_TF_SAME if same else POOL_TF_VALID, k, stride, 0, 0)
                else:
                    geom = (POOL_TORCH, 2, 2, 0, 0)
                L.append(Layer("pool:%d" % n_pool, "pool", pool(geom[0], geom[1], geom[2], geom[3], False), (cur, NONE, NONE), pool=geom))
                cur, n_pool, idx = len(L) - 1, n_pool + 1, idx + 1
            elif v == "D":
                idx += 1
            else:
                key = "%s.%s.%d" % (root, lname, idx)
                bn = "%s.%s.%d" % (root, lname, idx + 2)
                has_bn = bn + ".running_mean" in sd
                s2, b2 = fold_bn(sd, bn, 1e-3) if has_bn else (None, None)
                w = sd[key + ".weight"]
                L.append(Layer(key, "conv", plain_conv(w, sd[key + ".bias"], s2, b2, wround=wround, mutate=mutate), (cur, NONE, NONE),
                               K=int(np.prod(w.shape[1:])), steps=4 if has_bn else 0, weights=(key + ".weight",)))
                cur, idx = len(L) - 1, idx + (3 if has_bn else 2)
    if head_w is not None:
        hw = _d(head_w)
        L.append(Layer("head", "head", head(hw[:, :, None, None], head_bias, wround=wround), (cur, NONE, NONE), K=hw.shape[1]))
    return L


def deeplab_layers(weights):
    """the trunk of the SEC / DSRG DeepLab-VGG16 (tests/deeplab_ref.forward up to pool5a); weights {layer: {'w' HWIO, 'b'}}"""
    L = []
    cur, n_pool = INPUT, 0

    def add_pool(stride, avg):
        nonlocal cur, n_pool
        L.append(Layer("pool:%d" % n_pool, "pool", pool(POOL_TF_SAME, 3, stride, 0, avg), (cur, NONE, NONE), pool=(POOL_TF_SAME, 3, stride, 0, int(avg))))
        cur, n_pool = len(L) - 1, n_pool + 1

    for name in deeplab_ref.TRUNK:
        w = _d(weights[name]["w"]).permute(3, 2, 0, 1).contiguous()  # HWIO -> OIHW
        dil = 2 if name.startswith("conv5") else 1
        L.append(Layer(name, "conv", plain_conv(w, weights[name]["b"], None, None, pad=dil, dil=dil), (cur, NONE, NONE),
                       K=int(np.prod(w.shape[1:])), weights=(name + ".w",)))
        cur = len(L) - 1
        if name in ("conv1_2", "conv2_2", "conv3_3"):
            add_pool(2, False)
        elif name in ("conv4_3", "conv5_3"):
            add_pool(1, False)
    add_pool(1, True)
    return L


def chain(layers, x):
    """every layer's output from the network input x (NCHW double), in double: the whole forward pass through the closures"""
    outs = []
    for ly in layers:
        a, b, c = [x if i == INPUT else (None if i == NONE else outs[i]) for i in ly.inputs]
        y = ly.fn(a, b, c)[0]
        if ly.concat_with is not None:
            y = torch.cat([outs[ly.concat_with], y], 1)
        outs.append(y)
    return outs


def conv_weight_keys(sd):
    """the keys of a state dict that are convolution weights (4-D '.weight' / '.w')"""
    return sorted(k for k, v in sd.items() if (k.endswith(".weight") or k.endswith(".w")) and np.asarray(v).ndim == 4)


def extreme_bn_state_dict(num_classes=20, seed=4):
    """the BatchNorm scales of tests/test_gpu_edge.py::test_stage_entry_fusion_with_extreme_batchnorm_scales on every stage entry:
    zero bn3, zero shortcut scale, both, negative scales, scales five orders of magnitude apart in one channel"""
    sd = cnn_ref.make_resnet50_cam_state_dict(num_classes, seed=seed)
    for li in (1, 2, 3, 4):
        w3, wd = sd["resnet50.layer%d.0.bn3.weight" % li], sd["resnet50.layer%d.0.downsample.1.weight" % li]
        n = w3.numel()
        w3[0:n // 8] = 0.0
        wd[n // 16:n // 8 + n // 16] = 0.0
        w3[n // 4:n // 4 + n // 8] *= -1.0
        wd[n // 2:n // 2 + n // 8] *= -1.0
        w3[3 * n // 4:3 * n // 4 + n // 16] *= 1e-5
        wd[7 * n // 8:7 * n // 8 + n // 16] *= 1e-5
    return sd


def odd_s2_state_dict(num_classes=20, seed=5):
    """VGG16-BN whose post-ReLU BatchNorm scale is negative on some channels and tiny on others"""
    sd = cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, num_classes, True, seed=seed)
    for k in [k for k in sd if k.endswith(".running_mean")]:
        g = sd[k[:-len("running_mean")] + "weight"]
        n = g.numel()
        g[0:n // 8] *= -1.0
        g[n // 4:n // 4 + n // 8] *= 1e-4
        g[n // 2:n // 2 + n // 16] *= -1e-3
    return sd


# ---- the bound of a conv / head entry --------------------------------------------------------------------------------------------
U = 2.0 ** -24  # unit round-off of fp32
# what the single-layer tests hold the same launcher to (tests/test_gpu_conv.py): (relative to |ref|, relative to max|ref|)
SINGLE_LAYER = {"f16x3": (0.0, 4e-6), "bf16x3": (0.0, 1e-4), "f16": (2.0 ** -11, 3e-4)}


def derived_bound(prec, layer, ref, A, S, f32_out=False):
    """Per element, from the arithmetic (all terms in float64 numpy):
      every mode   the fp32 accumulation: a chain of P K additions (P = 1 product per weight, 3 in the split modes: hi hi, lo hi,
                   hi lo) -- plus 8 for the epilogue (the fp32 roundings of the folded scale and shift, their multiply and add, the
                   margin tests/test_gpu_f32.py's (K + 8) 2^-24 A carries) plus `steps`: one per extra epilogue step (residual add;
                   second affine: its fp32 scale, shift, multiply, add; stage entry: sigma, s / sigma, b3 + bd) -- each relative to A
      f32          nothing else: (K + 8 + steps) 2^-24 A
      f16x3        + 2^-22 A     the weight hi + lo pair holds 22 bits (the traced activation pair IS the operand: no term)
                   + 2 2^-24 A   stage entry only: w s / sigma is rounded to fp32 twice before it is split
                   + 2^-22 A     the dropped lo lo product: |x_lo| <= 2^-11 |x|, |w_lo| <= 2^-11 |w|
                   + 2^-37 S     a weight lo below half's normal range (weights are scaled so that the channel's largest is in
                                 [2^12, 2^13); half's subnormal spacing 2^-24 leaves 2^-25 absolute = 2^-37 of that maximum)
                   + 2^-22 |ref| + 2^-25  the output's own split (lo is a half: relative 2^-11 of a 2^-11 remainder; absolute
                                 half a subnormal spacing where lo is subnormal); not for an fp32 output (the head)
      bf16x3       the same with 2^-16 for 2^-22 (8 + 8 bits) and no subnormal terms (bfloat16 has fp32's exponent range)
      f16          against a reference FED the rounded weights: the chain, + 2^-11 |ref| + 2^-25 for the output's rounding"""
    P = 1 if prec in ("f32", "f16") else 3
    rel = (P * layer.K + 8 + layer.steps) * U
    b = np.zeros_like(ref)
    if prec == "f16x3":
        rel += 2.0 ** -22 + 2.0 ** -22 + (2 * U if layer.entry else 0.0)
        b = 2.0 ** -37 * S + (0.0 if f32_out else 2.0 ** -22 * np.abs(ref) + 2.0 ** -25)
    elif prec == "bf16x3":
        rel += 2.0 ** -16 + 2.0 ** -16 + (2 * U if layer.entry else 0.0)
        b = 0.0 if f32_out else 2.0 ** -16 * np.abs(ref)
    elif prec == "f16":
        b = 0.0 if f32_out else 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return rel * A + b


def asserted_bound(prec, layer, ref, A, S, f32_out=False, ref_max=None):
    """min(derived, the single-layer tests' bound) per element; f32 has the derived bound alone.  -> (bound, derived, table)"""
    d = derived_bound(prec, layer, ref, A, S, f32_out)
    if prec == "f32":
        return d, d, None
    r, m = SINGLE_LAYER[prec]
    t = r * np.abs(ref) + m * (np.abs(ref).max() if ref_max is None else ref_max)
    return np.minimum(d, t), d, t
