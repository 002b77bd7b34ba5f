"""03a_sec-dsrg mirror: the two host `py_func`s its training graph calls on every step, on libwsscam.

    generate_seed_step   DSRG.py:356-369 (and single_generate_seed_step :7-62 behind its process pool)
    crf_layer            the `crf` closure of DSRG.py:323-332 / SEC.py:270-280

The TF graph and the training of SEC / DSRG are out of scope; a DSRG model binds these two in place of the
closures it hands to tf.py_func and needs neither the process pool nor pydensecrf."""
import numpy as np

from . import _lib
from .misc.imutils import default_context


def generate_seed_step(tags, cues, probs, ctx=None, th_f=0.5, th_b=0.7):
    """DSRG seeded region growing of a batch (wsc_dsrg_seed_grow): one upload, one call, one download.

    tags  (B, C) or (B, 1, 1, C) float 0/1 image-level labels, class 0 = background
    cues  (B, H, W, C) float 0/1 seed cues
    probs (B, H, W, C) softmax
    -> float32 (B, H, W, C): the cues after growing.

    Returns a NEW array and leaves its inputs unmodified.  The reference mutates `cues` through a view (`cue[x, y, c] = 1`
    on `cues[i]`, DSRG.py:61) and returns the concatenation of those views' copies; a caller that relied on the side effect
    assigns the result back."""
    ctx = ctx or default_context()
    cues_f = np.ascontiguousarray(cues, dtype=np.float32)
    probs_f = np.ascontiguousarray(probs, dtype=np.float32)
    if cues_f.ndim != 4 or probs_f.shape != cues_f.shape:
        raise ValueError("generate_seed_step: cues %r and probs %r must both be (B, H, W, C)" % (np.shape(cues), np.shape(probs)))
    B, H, W, C = cues_f.shape
    tags_f = np.ascontiguousarray(tags, dtype=np.float32)
    if tags_f.shape not in ((B, C), (B, 1, 1, C)):
        raise ValueError("generate_seed_step: tags %r must be (B, C) or (B, 1, 1, C) for cues %r" % (tags_f.shape, cues_f.shape))
    # one buffer [tags | cues | probs]: one copy in, grown in place, one copy out
    n = cues_f.size
    packed = np.concatenate([tags_f.reshape(-1), cues_f.reshape(-1), probs_f.reshape(-1)])
    buf = ctx.to_device(packed, pooled=True)
    try:
        cues_dev = buf.ptr + 4 * tags_f.size
        _lib.dsrg_seed_grow(ctx, buf.ptr, cues_dev, cues_dev + 4 * n, B, H, W, C, cues_dev, th_f=th_f, th_b=th_b)
        return ctx.to_host(cues_dev, (B, H, W, C), np.float32)
    finally:
        buf.free()


def crf_layer(featmap, image, crf_config, num_classes, min_prob=1e-4, ctx=None, return_q=False):
    """The dense-CRF layer of SEC / DSRG: lib.crf.crf_inference(image[i], crf_config, num_classes, featmap[i],
    use_log=True) for every image of the batch, then clamp at min_prob, renormalise over classes and take the log.

    featmap (B, H, W, C) softmax at the seed size;  image (B, H, W, 3), cast to uint8 as the reference does.
    ONE wsc_crf over the B images and one mean-field loop (the reference builds B CRFs, one per image).
    -> float32 (B, H, W, C) log-probabilities; with return_q also the marginals (B, H, W, C) before that tail."""
    ctx = ctx or default_context()
    fm = np.asarray(featmap, dtype=np.float32)
    B, H, W, C = fm.shape
    if C != num_classes:
        raise ValueError("crf_layer: featmap has %d classes, num_classes = %d" % (C, num_classes))
    img = np.ascontiguousarray(np.asarray(image).astype(np.uint8))
    if img.shape != (B, H, W, 3):
        raise ValueError("crf_layer: image %r must be (B, H, W, 3) at the featmap's size %r" % (img.shape, fm.shape))
    U = np.ascontiguousarray(np.transpose(-np.log(fm), (0, 3, 1, 2)))  # [B][C][H*W]
    rgb_dev = ctx.to_device(img, pooled=True)
    u_dev = ctx.to_device(U, pooled=True)
    q_dev = ctx.alloc(U.nbytes, pooled=True)
    crf = _lib.Crf(ctx, rgb_dev, B, H, W, crf_config["g_sxy"], crf_config["bi_sxy"], crf_config["bi_srgb"])
    try:
        crf.inference(u_dev, C, crf_config["g_compat"], crf_config["bi_compat"], int(crf_config["iterations"]), q_dev, None)
        q = np.ascontiguousarray(np.transpose(ctx.to_host(q_dev, (B, C, H, W), np.float32), (0, 2, 3, 1)))
    finally:
        crf.close()
        for d in (rgb_dev, u_dev, q_dev):
            d.free()
    ret = q.copy()
    ret[ret < min_prob] = min_prob
    ret /= np.sum(ret, axis=3, keepdims=True)
    ret = np.log(ret).astype(np.float32)
    return (ret, q) if return_q else ret
