"""HistoSegNet post-processing on the device -- mirror of 03c_hsn/utilities.py.

dcrf_process :399-445 is the only in-tree pydensecrf call site; here the whole batch goes
through libwsscam's permutohedral mean-field in one call per distinct class count."""
import numpy as np

from .. import _lib
from ..cues import utilities as cues_utilities
from ..misc.imutils import default_context, unary_from_softmax


def grad_cam_device(input_model, weights, images, thresholds, orig_sz, raw_u8=None, mean_std=None, out=None, ctx=None,
                    chain=None):
    """HSN grad_cam with everything after the batch upload on the device: one CNN pass (einsum maps + scores,
    SURVEY Q9), score gate, per-map upsample + max(., 0), per-image normalisation (03c_hsn/utilities.py:258-277 with
    the class gating of demo.py:127-131 / :335-341).  `images`: normalised (B,S,S,3) floats, or None with `raw_u8`
    (B,S,S,3) uint8 + `mean_std` = (mean[3] or scalar, std[3] or scalar): the normalisation runs on the device as well
    (wsc_msf_input_u8).  `out` = (buffer, channels, first): write the maps into channels [first, first + C) of a wider
    [B][channels][S*S] stack.  Returns (H_dev [B][C][S*S] device buffer, scores (B, C), is_pass (B, C), ctx[, raw_dev]);
    H stays in HBM for wsc_hsn_cs_gradcam / the CRF."""
    net, nctx = input_model.gradcam_net(np.asarray(weights), ctx=ctx)
    ctx = nctx
    raw_dev = None
    if images is None:
        B, S_in = raw_u8.shape[0], raw_u8.shape[1]
        raw_dev = ctx.to_device(raw_u8, pooled=True)
        x_dev = ctx.alloc(B * 3 * S_in * S_in * 4, pooled=True)
        mean = np.broadcast_to(np.asarray(mean_std[0], np.float32), (3,))
        std = np.broadcast_to(np.asarray(mean_std[1], np.float32), (3,))
        _lib.msf_input_u8(ctx, raw_dev, [(S_in, S_in)] * B, np.arange(B, dtype=np.int64) * (S_in * S_in * 3), S_in,
                          mean, std, x_dev, pre_div255=False, pair=False)
    else:
        x = cues_utilities._to_nchw(images)
        B, S_in = x.shape[0], x.shape[2]
        x_dev = ctx.to_device(x, pooled=True)
    h = net.cam_size(S_in)
    C = np.asarray(weights).shape[1]
    S = int(orig_sz[0])
    assert int(orig_sz[1]) == S, "square output size"
    cams_dev = ctx.alloc(B * h * h * C * 4, pooled=True)
    score_dev = ctx.alloc(B * C * 4, pooled=True)
    if chain is not None:  # (a driver with several batches in flight: one conv stack at a time, _lib.StackChain)
        chain.run(ctx, lambda: net.forward_gradcam(x_dev, B, S_in, False, cams_dev, score_dev, ctx=ctx))
    else:
        net.forward_gradcam(x_dev, B, S_in, False, cams_dev, score_dev, ctx=ctx)
    scores = ctx.to_host(score_dev, (B, C), np.float32)  # 4 B C bytes: the gate is a host decision in the reference too
    is_pass = np.greater_equal(scores, np.asarray(thresholds).reshape(1, -1))
    gate_dev = ctx.to_device((scores * is_pass).astype(np.float32), pooled=True)
    if out is None:
        H_dev = ctx.alloc(B * C * S * S * 4, pooled=True)
        _lib.hsn_gradcam_post(ctx, cams_dev, B, h, h, C, S, gate_dev, H_dev)
    else:
        H_dev = out[0]
        _lib.hsn_gradcam_post(ctx, cams_dev, B, h, h, C, S, gate_dev, H_dev, out_channels=out[1], out_first=out[2])
    if raw_dev is not None:
        return H_dev, scores, is_pass, ctx, raw_dev
    return H_dev, scores, is_pass, ctx


def grad_cam(input_model, weights, images, is_pass_threshold, final_layer, conf_scores, orig_sz=[224, 224],
             should_upsample=False):
    """03c_hsn/utilities.py:231-278 -> (B, S, S, C): einsum (no ReLU before the resize), per-map bilinear
    upsample then max(., 0), division by the per-image maximum over all classes, gating by score x pass.
    numpy in / numpy out like the reference; the arithmetic runs in wsc_net_forward_gradcam + wsc_hsn_gradcam_post."""
    net, ctx = input_model.gradcam_net(np.asarray(weights))
    x = cues_utilities._to_nchw(images)
    B, S_in = x.shape[0], x.shape[2]
    h = net.cam_size(S_in)
    C = np.asarray(weights).shape[1]
    cams_dev = ctx.alloc(B * h * h * C * 4, pooled=True)
    net.forward_gradcam(ctx.to_device(x, pooled=True), B, S_in, False, cams_dev, None)
    if not should_upsample:  # (no reference caller; kept for the signature) normalise at the CNN resolution
        cams = ctx.to_host(cams_dev, (B, h, h, C), np.float32).astype(np.float64)
        cams = cams / np.maximum(np.max(cams, axis=(1, 2, 3), keepdims=True), 1e-7)
        return cams * np.expand_dims(np.expand_dims(conf_scores * is_pass_threshold, axis=1), axis=2)
    S = int(orig_sz[0])
    gate_dev = ctx.to_device(np.ascontiguousarray(np.asarray(conf_scores) * np.asarray(is_pass_threshold), dtype=np.float32), pooled=True)
    out_dev = ctx.alloc(B * C * S * S * 4, pooled=True)
    _lib.hsn_gradcam_post(ctx, cams_dev, B, h, h, C, S, gate_dev, out_dev)
    out = ctx.to_host(out_dev, (B, C, S, S), np.float32)
    return np.transpose(out, (0, 2, 3, 1)).astype(np.float64)


def _htt_tables(classes, func):
    exceptions = ["G.O", "G.N", "T"] if func else ["A.W", "A.B", "A.M"]
    return classes.index("Background"), (classes.index("Other") if func else -1), \
        [i for i, c in enumerate(classes) if c in exceptions]


def modify_by_htt(gradcam, images, classes, gradcam_adipose=None, ctx=None):
    """03c_hsn/utilities.py:306-364: synthesise the 'Background' (and, for functional types, 'Other')
    channels of an ADP Grad-CAM stack in place and return it.

    background = 0.75 * sigmoid(4 * (mean_rgb - 240)), Gaussian-smoothed (sigma 2), minus the strongest
    exception-class activation; other = max(0.05 * (1 - max_c cam), adipose cam).  numpy in / numpy out; the work is
    wsc_hsn_background + wsc_hsn_cs_gradcam on the device (the drivers call those directly and never come here)."""
    ctx = ctx or default_context()
    gradcam = np.asarray(gradcam)
    B, Cv, Hh, Ww = gradcam.shape
    Hi, Wi = int(np.asarray(images).shape[1]), int(np.asarray(images).shape[2])
    func = gradcam_adipose is not None
    bg_ind, other_ind, ex_inds = _htt_tables(list(classes), func)
    stack = gradcam.astype(np.float32)
    adip = None
    if func:
        na = gradcam_adipose.shape[1]
        stack = np.concatenate((stack, np.asarray(gradcam_adipose, dtype=np.float32)), axis=1)
        adip = list(range(Cv, Cv + na))
    N = Hh * Ww
    H_dev = ctx.to_device(np.ascontiguousarray(stack.reshape(B, -1, N)), pooled=True)
    bg_dev = ctx.alloc(B * N * 8, pooled=True)
    _lib.hsn_background(ctx, ctx.to_device(np.ascontiguousarray(np.uint8(images)), pooled=True), B, Hi, Wi, bg_dev, out_hw=(Hh, Ww))
    cs_dev, y_dev, mass_dev = ctx.alloc(B * Cv * N * 4, pooled=True), ctx.alloc(B * Cv * N * 4, pooled=True), ctx.alloc(B * Cv * 4, pooled=True)
    _lib.hsn_cs_gradcam(ctx, H_dev, B, stack.shape[1], N, bg_dev, list(range(Cv)), bg_ind, other_ind, ex_inds, adip, cs_dev,
                        y_dev, mass_dev)
    y = ctx.to_host(y_dev, (B, Cv, Hh, Ww), np.float32)
    gradcam[:, bg_ind] = y[:, bg_ind]  # only the synthesised channels are written, as in the reference (:349, :362)
    if func:
        gradcam[:, other_ind] = y[:, other_ind]
    return gradcam


def get_cs_gradcam(gradcam, classes, htt_class, ctx=None):
    """03c_hsn/utilities.py:367-397: class-specific Grad-CAM = (top1 - top2 margin) on the arg-max class,
    zero elsewhere; the functional/glas 'Other' channel passes through unchanged.  (wsc_hsn_cs_gradcam, modify step off.)"""
    ctx = ctx or default_context()
    gradcam = np.asarray(gradcam)
    B, Cv, Hh, Ww = gradcam.shape
    N = Hh * Ww
    other_ind = list(classes).index("Other") if htt_class in ("func", "glas") else -1
    H_dev = ctx.to_device(np.ascontiguousarray(gradcam.reshape(B, Cv, N), dtype=np.float32), pooled=True)
    cs_dev, mass_dev = ctx.alloc(B * Cv * N * 4, pooled=True), ctx.alloc(B * Cv * 4, pooled=True)
    _lib.hsn_cs_gradcam(ctx, H_dev, B, Cv, N, None, list(range(Cv)), 0, other_ind, [], None, cs_dev, None, mass_dev)
    return ctx.to_host(cs_dev, (B, Cv, Hh, Ww), np.float32).astype(gradcam.dtype if gradcam.dtype.kind == "f" else np.float64)


def dcrf_process_device(ctx, cs_dev, mass, rgb_host, Cv, H, W, config, keep_dev=None):
    """dcrf_process (03c_hsn/utilities.py:399-445) on class-specific maps that are already in HBM: per image the
    classes with positive mass (`mass` (B, Cv) from wsc_hsn_cs_gradcam, :425), unaries gathered on the device (:431),
    ONE ragged CRF object for the batch -- every image runs with its own class count len(pass_inds[i]), as the reference's
    per-image DenseCRF2D does (wsc_crf_v; round 3 ran one wsc_crf per distinct class count: 13 loops for 16 patches) --
    and the arg-max mapped back through each image's class list.  -> (B, H, W) int64.
    keep_dev: a list that receives (the uint8 label maps on the device, one H x W map per image of `idxs`, back to back; idxs) --
    what the debug-image renderer starts from; nothing is appended when no image has a passing class."""
    gauss_sxy, gauss_compat, bilat_sxy, bilat_srgb, bilat_compat, n_infer = config
    B = mass.shape[0]
    N = H * W
    out = np.zeros((B, H, W), np.int64)  # an image without a passing class: arg-max of an all-zero stack = 0
    pass_inds = [np.nonzero(mass[i])[0] for i in range(B)]
    idxs = [i for i in range(B) if len(pass_inds[i]) > 0]
    if not idxs:
        return out
    Bv = len(idxs)
    Ms = [len(pass_inds[i]) for i in idxs]
    chan = [(i * Cv + int(c)) * N for i in idxs for c in pass_inds[i]]
    u_dev = ctx.alloc(sum(Ms) * N * 4, pooled=True)
    _lib.hsn_gather_unary(ctx, cs_dev, chan, N, u_dev)
    row0 = np.concatenate(([0], np.cumsum(Ms)))
    rgb_dev = ctx.to_device(np.ascontiguousarray(rgb_host[idxs]), pooled=True)
    a_dev = ctx.alloc(Bv * N * 4, pooled=True)
    d = _lib.CrfV(ctx, [rgb_dev.ptr + j * N * 3 for j in range(Bv)], [(H, W)] * Bv, gauss_sxy, bilat_sxy, bilat_srgb)
    try:
        d.inference([u_dev.ptr + int(row0[j]) * N * 4 for j in range(Bv)], Ms, gauss_compat, bilat_compat, int(n_infer), None,
                    [a_dev.ptr + j * N * 4 for j in range(Bv)])
        # arg-max -> class index through each image's list of passing classes, on the device (a lookup table per image,
        # padded to the longest list: an arg-max never points into the padding); one uint8 read-back for the batch
        keys = np.zeros((Bv, max(Ms)), np.int64)
        for j, i in enumerate(idxs):
            keys[j, :Ms[j]] = pass_inds[i]
        conf_dev = ctx.alloc(Bv * N, pooled=True)
        _lib.ir_label_combine(ctx, a_dev, None, keys, N, conf_dev)
        out[idxs] = ctx.to_host(conf_dev, (Bv, H, W), np.uint8)
        if keep_dev is not None:
            keep_dev.append((conf_dev, idxs))
    finally:
        d.close()
    return out


def dcrf_process(probs, images, config, ctx=None):
    """Run dense CRF, given probability map and input image (03c_hsn/utilities.py:399-445).

    probs  : (B, C, H, W) class probability maps
    images : (B, H, W, 3) original input images
    config : [g_sxy, g_compat, bi_sxy, bi_srgb, bi_compat, n_infer]
    returns (B, H, W) int64 arg-max class map.
    """
    gauss_sxy, gauss_compat, bilat_sxy, bilat_srgb, bilat_compat, n_infer = config
    ctx = ctx or default_context()
    probs = np.asarray(probs)
    num_input_images, num_classes = probs.shape[0], probs.shape[1]
    size = images.shape[1:3]
    H, W = int(size[0]), int(size[1])
    crf = np.zeros((num_input_images, num_classes, H, W))
    # per image: classes with any positive mass (:425)
    pass_inds = [np.where(np.sum(np.sum(probs[i], axis=1), axis=1) > 0)[0] for i in range(num_input_images)]
    rgb = np.ascontiguousarray(np.uint8(images))
    # images sharing a class count M go through the device together
    groups = {}
    for i, p in enumerate(pass_inds):
        if len(p) > 0:
            groups.setdefault(len(p), []).append(i)
    for M, idxs in groups.items():
        Bg = len(idxs)
        U = np.stack([np.ascontiguousarray(unary_from_softmax(probs[i, pass_inds[i]])) for i in idxs])
        rgb_dev = ctx.to_device(rgb[idxs], pooled=True)
        u_dev = ctx.to_device(U.astype(np.float32), pooled=True)
        q_dev = ctx.alloc(Bg * M * H * W * 4, pooled=True)
        d = _lib.Crf(ctx, rgb_dev, Bg, H, W, gauss_sxy, bilat_sxy, bilat_srgb)
        d.inference(u_dev, M, gauss_compat, bilat_compat, int(n_infer), q_dev, None)
        Q = ctx.to_host(q_dev, (Bg, M, H, W), np.float32)
        d.close()
        for j, i in enumerate(idxs):
            crf[i, pass_inds[i]] = Q[j]
    maxconf_crf = np.argmax(crf, axis=1)
    return maxconf_crf
