"""TEST INFRASTRUCTURE ONLY (oracle) -- the Keras-side CAM nets with the MaxPooling2D geometry of a session's architecture
file, on torch CPU: oracle/cnn_ref.py's plain_features / vgg16_cam_forward / m7_cam_forward / grad_cam_weights restated with
every F.max_pool2d(x, 2, 2) replaced by TensorFlow's pool of one (k, stride, 'same' | 'valid') row.

TensorFlow's rule per axis (tests/deeplab_ref.same_pad is the SAME half of it):
  'same'   out = ceil(n / stride), pad_total = max((out - 1) stride + k - n, 0), pad_before = floor(pad_total / 2)
  'valid'  out = floor((n - k) / stride) + 1, no padding
The padding is -inf (explicit F.pad), so it never wins a maximum; F.max_pool2d(k, stride) on the padded tensor is then VALID."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn_ref
from tests import deeplab_ref


def tf_pool_axis(n, k, stride, same):
    """-> (out, pad_before, pad_after)"""
    if same:
        return deeplab_ref.same_pad(n, stride, k)
    if n < k:
        raise ValueError("a VALID window of %d does not fit %d positions" % (k, n))
    return (n - k) // stride + 1, 0, 0


def tf_max_pool_t(t, k, stride, same):
    """NCHW tensor -> its TF max pool"""
    ho, pt, pb = tf_pool_axis(t.shape[2], k, stride, same)
    wo, pl, pr = tf_pool_axis(t.shape[3], k, stride, same)
    y = F.max_pool2d(F.pad(t, (pl, pr, pt, pb), value=float("-inf")), k, stride)
    assert tuple(y.shape[2:]) == (ho, wo), (tuple(y.shape), ho, wo)
    return y


def tf_max_pool(x, k, stride, same, dtype=torch.float64):
    """NHWC numpy -> NHWC numpy of `dtype`"""
    t = torch.as_tensor(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2)
    return tf_max_pool_t(t, k, stride, same).permute(0, 2, 3, 1).contiguous().numpy()


def _row(row):
    k, stride, padding = row
    assert padding in ("same", "valid")
    return int(k), int(stride), padding == "same"


def plain_features_pooled(x, sd, root, cfg, pools, return_pre_bn=False):
    """cnn_ref.plain_features with the i-th 'M' entry pooled by pools[i]"""
    pre = None
    n_pool = 0
    for lname, layer in cfg:
        idx = 0
        for v in layer:
            if v == "M":
                x = tf_max_pool_t(x, *_row(pools[n_pool]))
                n_pool += 1
                idx += 1
            elif v == "D":
                idx += 1
            else:
                key = "%s.%s.%d" % (root, lname, idx)
                x = F.relu(F.conv2d(x, sd[key + ".weight"], sd[key + ".bias"], padding=1))
                pre = x
                bn = "%s.%s.%d" % (root, lname, idx + 2)
                if bn + ".running_mean" in sd:
                    x = cnn_ref._fixed_bn(x, sd, bn, eps=1e-3)
                    idx += 3
                else:
                    idx += 2
    return (x, pre) if return_pre_bn else x


def vgg16_cam_forward(x, sd, num_classes, pools):
    """cnn_ref.vgg16_cam_forward on the pooled stack: (cam (C, h, w), score (C,))"""
    x = plain_features_pooled(x, sd, "vgg16", cnn_ref.VGG16_CFG, pools)
    y = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    y = torch.sigmoid(F.linear(y, sd["vgg16.classifier.0.weight"], sd.get("vgg16.classifier.0.bias")))[0]
    cam = F.relu(F.conv2d(x, sd["vgg16.classifier.0.weight"][:num_classes].unsqueeze(-1).unsqueeze(-1)))
    return cam[0] + cam[1].flip(-1), y[:num_classes]


def m7_cam_forward(x, sd, gradcam_weights, num_classes, pools, crop=True):
    """cnn_ref.m7_cam_forward on the pooled stack; the classifier branch pools with pools[2] before its global max.
    crop=False: the global max of the UNPOOLED map instead (what a pool that covers every position gives anyway)."""
    x = plain_features_pooled(x, sd, "m7", cnn_ref.M7_CFG, pools[:2])
    y = tf_max_pool_t(x, *_row(pools[2])) if crop else x
    y = torch.flatten(F.adaptive_max_pool2d(y, (1, 1)), 1)
    y = torch.sigmoid(F.linear(y, sd["m7.classifier.0.weight"], sd.get("m7.classifier.0.bias")))[0]
    w = gradcam_weights.float()
    cam = F.relu(F.conv2d(x, w.transpose(1, 0).unsqueeze(-1).unsqueeze(-1)))
    return cam[0] + cam[1].flip(-1), y[:num_classes]


def grad_cam_weights(sd, root, cfg, S, num_classes, pools):
    """cnn_ref.grad_cam_weights (autograd on a zeros image, A = the final Activation's output) on the pooled stack"""
    x = torch.zeros(1, 3, S, S)
    n_stack = sum(1 for _, layer in cfg for v in layer if v == "M")
    with torch.no_grad():
        _, pre = plain_features_pooled(x, sd, root, cfg, pools[:n_stack], return_pre_bn=True)
    A = pre.detach().requires_grad_(True)
    bn = cnn_ref.last_bn_key(sd, root, cfg)
    feat = cnn_ref._fixed_bn(A, sd, bn, eps=1e-3) if bn else A
    if root == "m7":
        pooled = torch.flatten(F.adaptive_max_pool2d(tf_max_pool_t(feat, *_row(pools[n_stack])), (1, 1)), 1)
    else:
        pooled = torch.flatten(F.adaptive_avg_pool2d(feat, (1, 1)), 1)
    logits = F.linear(pooled, sd[root + ".classifier.0.weight"], sd.get(root + ".classifier.0.bias"))[0]
    alpha = np.zeros((A.shape[1], num_classes))
    for c in range(num_classes):
        (g,) = torch.autograd.grad(logits[c], A, retain_graph=True)
        g = g / (torch.sqrt(torch.mean(g * g)) + 1e-5)
        alpha[:, c] = g[0].mean(dim=(1, 2)).numpy()
    return alpha


# ---- Keras 2 `model.to_json()` documents of the two model types, as a session's <sess_id>.json holds them --------------------
def keras_layers(root, pools, batchnorm, use_bias, num_classes=20):
    """The layer list of the Sequential model: Conv2D -> Activation -> [BatchNormalization] per conv entry, the pools of
    `pools` at the 'M' positions (M7: its third before the global pooling), Dropout at 'D', global pooling, Dense."""
    cfg = cnn_ref.VGG16_CFG if root == "vgg16" else cnn_ref.M7_CFG
    out = []
    n_pool = 0

    def pool(row):
        k, stride, padding = row
        return {"class_name": "MaxPooling2D", "config": {"name": "max_pooling2d_%d" % (n_pool + 1), "pool_size": [k, k],
                                                         "strides": [stride, stride], "padding": padding,
                                                         "data_format": "channels_last"}}

    for _, layer in cfg:
        for v in layer:
            if v == "M":
                out.append(pool(pools[n_pool]))
                n_pool += 1
            elif v == "D":
                out.append({"class_name": "Dropout", "config": {"rate": 0.5}})
            else:
                out.append({"class_name": "Conv2D", "config": {"filters": v, "kernel_size": [3, 3], "strides": [1, 1],
                                                               "padding": "same", "dilation_rate": [1, 1], "activation": "linear",
                                                               "use_bias": True}})
                out.append({"class_name": "Activation", "config": {"activation": "relu"}})
                if batchnorm:
                    out.append({"class_name": "BatchNormalization", "config": {"axis": -1, "momentum": 0.99, "epsilon": 0.001}})
    if root == "m7":
        out.append(pool(pools[n_pool]))
        out.append({"class_name": "Dropout", "config": {"rate": 0.5}})
    out.append({"class_name": "GlobalAveragePooling2D" if root == "vgg16" else "GlobalMaxPooling2D", "config": {}})
    out.append({"class_name": "Dense", "config": {"units": num_classes, "activation": "sigmoid", "use_bias": use_bias}})
    return out


def keras_document(layers, container="list", class_name="Sequential"):
    """container 'list': "config": [layers]; 'dict': "config": {"name", "layers": [layers]} (both are Keras 2 forms)"""
    cfg = list(layers) if container == "list" else {"name": "sequential_1", "layers": list(layers)}
    return {"class_name": class_name, "config": cfg, "keras_version": "2.2.4", "backend": "tensorflow"}
