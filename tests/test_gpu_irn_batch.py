"""GPU: the IRNet training-sample transform on the device (csrc/irn_batch.hip: wsc_pil_resize_u8, wsc_irn_train_batch;
irn_train.TrainBatcher; step.train_irn.run) against tests/irn_batch_ref.py, the numpy restatement that
tests/test_irn_batch_oracle.py pins against PIL's Image.resize itself.  Every comparison is an equality of bytes or bits.

Every device buffer a kernel reads or writes here -- the packed images and labels, the three outputs, the resize's result --
lies between 4 KiB of sentinel bytes, which must be intact afterwards."""
import types

import numpy as np
import pytest

from tests import irn_batch_ref as ref
from tests.test_irn_batch_oracle import synthetic_dataset
from wsscam import _lib, irn_train, synth
from wsscam.misc.indexing import PathIndex
from wsscam.net import resnet50_irn
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0xA5
VOC_INT = ((104.0, 117.0, 123.0), (255.0, 255.0, 255.0))
VOC_FLOAT = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


class Guarded:
    """`nbytes` of device memory between two sentinel bands; payload: the bytes to upload (else sentinels as well)"""

    def __init__(self, ctx, nbytes, payload=None):
        host = np.full(GUARD + nbytes + GUARD, SENTINEL, np.uint8)
        if payload is not None:
            host[GUARD:GUARD + nbytes] = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
        self.nbytes = nbytes
        self.maps = DeviceMaps.from_host(ctx, host)
        self.ptr = self.maps.ptr + GUARD

    def payload(self, what, dtype=np.uint8):
        host = self.maps.to_host()
        assert (host[:GUARD] == SENTINEL).all(), what + ": a store in front of the buffer"
        assert (host[GUARD + self.nbytes:] == SENTINEL).all(), what + ": a store behind the buffer"
        return host[GUARD:GUARD + self.nbytes].copy().view(dtype)

    def free(self):
        self.maps.free()


def _pack(arrays):
    offs = np.concatenate([[0], np.cumsum([a.size for a in arrays])]).astype(np.int64)
    return np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in arrays]), offs


# ---- wsc_pil_resize_u8 ----------------------------------------------------------------------------------------------------------------
def _resize_cases(channels):
    rng = np.random.default_rng(41)
    shape = (37, 53, 3) if channels == 3 else (37, 53)
    a = rng.integers(0, 256, shape).astype(np.uint8)
    yy, xx = np.mgrid[0:37, 0:53]
    board = (((yy // 2 + xx // 3) % 2) * 255).astype(np.uint8)  # 0 / 255: both clamps fire
    board = np.repeat(board[..., None], 3, 2) if channels == 3 else board
    tiny = rng.integers(0, 256, (2, 3, 3) if channels == 3 else (2, 3)).astype(np.uint8)
    return [(a, (19, 27)),      # support 4, 9 taps
            (a, (56, 80)),      # upscale
            (a, (37, 80)),      # the vertical pass skipped
            (a, (19, 53)),      # the horizontal pass skipped
            (tiny, (5, 2)),     # windows truncated on both sides
            (board, (19, 27)), (board, (56, 80)),
            (a, (37, 53))]      # the size kept: a copy


def _run_resize(ctx, cases, channels, order):
    images, offs = _pack([c[0] for c in cases])
    out_sizes = [c[1] for c in cases]
    out_offs = np.concatenate([[0], np.cumsum([h * w * channels for h, w in out_sizes])]).astype(np.int64)
    src, out = Guarded(ctx, images.size, images), Guarded(ctx, int(out_offs[-1]))
    try:
        _lib.pil_resize_u8(ctx, src.ptr, [c[0].shape[:2] for c in cases], offs[:-1], out_sizes, out_offs[:-1], channels, order, out.ptr)
        got = out.payload("resize result")
        assert np.array_equal(src.payload("packed images"), images)
    finally:
        src.free()
        out.free()
    return [got[out_offs[i]:out_offs[i + 1]].reshape(tuple(out_sizes[i]) + ((3,) if channels == 3 else ())) for i in range(len(cases))]


@pytest.mark.parametrize("channels,order", [(3, 3), (1, 0), (1, 3), (3, 0)])
def test_pil_resize_u8(ctx, channels, order):
    cases = _resize_cases(channels)
    got = _run_resize(ctx, cases, channels, order)
    clamped = [False, False]
    for (img, hw), g in zip(cases, got):
        want = ref.pil_bicubic(img, hw) if order == 3 else ref.pil_nearest(img, hw)
        assert np.array_equal(g, want), (img.shape, hw, int((g != want).sum()))
        if order == 3 and set(np.unique(img)) <= {0, 255} and hw[1] != img.shape[1]:
            for xmin, n, coef in ref.resample_coeffs(img.shape[1], hw[1]):
                acc = ((1 << 21) + np.tensordot(coef, img.reshape(37, 53, -1)[:, xmin:xmin + n].astype(np.int64), axes=(0, 1))) >> 22
                clamped = [clamped[0] or bool((acc < 0).any()), clamped[1] or bool((acc > 255).any())]
    assert order == 0 or clamped == [True, True]


# ---- wsc_irn_train_batch --------------------------------------------------------------------------------------------------------------
def _labels_for(rng, h, w):
    lab = rng.choice(np.array([0, 7, 20, 21, 255], np.uint8), (h // 3 + 1, w // 3 + 1)).repeat(3, 0).repeat(3, 1)[:h, :w]
    return np.ascontiguousarray(lab)


def _run_batch(ctx, images, labels, params, S, norm, pre_div255, stage, expect_error=False):
    """-> (x float32 (B,3,S,S), label uint8 (B,S,S), reduced uint8 (B,s,s)) from wsc_irn_train_batch on guarded buffers"""
    B, s = len(images), ref.reduced_size(S)
    img, ioff = _pack(images)
    lab, loff = _pack(labels)
    bufs = [Guarded(ctx, img.size, img), Guarded(ctx, lab.size, lab), Guarded(ctx, B * 3 * S * S * 4), Guarded(ctx, B * S * S), Guarded(ctx, B * s * s)]
    try:
        call = lambda: _lib.irn_train_batch(ctx, bufs[0].ptr, bufs[1].ptr, [i.shape[:2] for i in images], ioff[:-1], loff[:-1],  # noqa: E731
                                            np.asarray(params, np.int32), S, norm[0], norm[1], pre_div255, stage, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr)
        if expect_error:
            with pytest.raises(_lib.WscError) as ei:
                call()
            assert ei.value.status == _lib.WSC_ERR_INVALID
            ctx.sync()
            for b, what in zip(bufs[2:], ("x", "label", "reduced")):  # nothing was launched
                assert (b.payload(what) == SENTINEL).all(), what
            return str(ei.value)
        call()
        x = bufs[2].payload("x", np.float32).reshape(B, 3, S, S)
        label = bufs[3].payload("label").reshape(B, S, S)
        reduced = bufs[4].payload("reduced").reshape(B, s, s)
        assert np.array_equal(bufs[0].payload("packed images"), img) and np.array_equal(bufs[1].payload("packed labels"), lab)
        return x, label, reduced
    finally:
        for b in bufs:
            b.free()


def _check_batch(ctx, images, labels, params, S, norm, pre_div255, stage):
    got = _run_batch(ctx, images, labels, params, S, norm, pre_div255, stage)
    want = ref.batch(images, labels, params, S, norm[0], norm[1], pre_div255, stage)
    dx = got[0].view(np.uint32) != want[0].view(np.uint32)
    assert not dx.any(), ("x", int(dx.sum()), np.argwhere(dx)[:4].tolist())
    assert np.array_equal(got[1], want[1]), ("label", np.argwhere(got[1] != want[1])[:4].tolist())
    assert np.array_equal(got[2], want[2]), ("reduced", np.argwhere(got[2] != want[2])[:4].tolist())
    for b, p in enumerate(np.asarray(params)):  # the padding: exactly 0.0 (the +0.0 bits) and 255
        inside = np.zeros((S, S), bool)
        inside[p[3]:p[3] + p[7], p[4]:p[4] + p[8]] = True
        assert not got[0][b].view(np.uint32)[:, ~inside].any() and (got[1][b][~inside] == 255).all()
    return got


def _stage1_samples():
    """(source size, factor, flip, cont_top, cont_left, img_top, img_left) for S = 32; ch / cw follow"""
    return [((20, 25), 1.2, 1, 5, 2, 0, 0),      # 24 x 30: smaller than the crop on both axes, container offsets not 0
            ((50, 60), 0.9, 0, 0, 0, 9, 17),     # 45 x 54: larger, image offsets not 0
            ((50, 60), 0.5, 1, 4, 0, 0, 0),      # 25 x 30: the widest filter (support 4)
            ((20, 64), 1.0, 1, 7, 0, 0, 21),     # wider but shorter than the crop, factor 1.0: both passes skipped
            ((41, 27), 1.5, 0, 0, 0, 30, 3),     # 62 x 40 (np.round: 61.5 -> 62, 40.5 -> 40)
            ((33, 33), 1.3, 0, 0, 0, 11, 11)]    # 43 x 43


def _make_batch(samples, S, seed):
    rng = np.random.default_rng(seed)
    images, labels, params = [], [], []
    for (h, w), f, flip, ct, cl, it, il in samples:
        images.append(rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
        labels.append(_labels_for(rng, h, w))
        sh, sw = ref.scaled_size((h, w), f)
        params.append((sh, sw, flip, ct, cl, it, il, min(S, sh), min(S, sw)))
    return images, labels, np.array(params, np.int32)


@pytest.mark.parametrize("norm,pre", [(VOC_INT, False), (VOC_FLOAT, True)], ids=["int", "float"])
def test_train_batch_stage1(ctx, norm, pre):
    images, labels, params = _make_batch(_stage1_samples(), 32, 1)
    assert params[4].tolist()[:2] == [62, 40] and {0, 20, 21, 255} <= set(np.unique(np.concatenate([l.ravel() for l in labels])))
    x, label, reduced = _check_batch(ctx, images, labels, params, 32, norm, pre, 1)
    assert reduced.shape == (6, 8, 8) and np.array_equal(reduced, label[:, 2::4, 2::4])  # indices 2, 6, .., 30
    assert {0, 20, 21, 255} <= set(np.unique(label))


@pytest.mark.parametrize("S", [34, 30])
def test_train_batch_non_integral_reduction(ctx, S):
    samples = [((50, 60), 0.8, 1, 0, 0, 3, 5), ((20, 25), 1.1, 0, S - 22, S - 28, 0, 0)]
    images, labels, params = _make_batch(samples, S, S)
    x, label, reduced = _check_batch(ctx, images, labels, params, S, VOC_INT, False, 1)
    idx = ref.nearest_index(S, 8)
    assert reduced.shape == (2, 8, 8) and np.array_equal(reduced, label[:, idx][:, :, idx])
    assert idx.tolist()[-2:] == [27, 31] if S == 34 else idx.tolist()[:3] == [1, 5, 9]


def test_train_batch_stage2(ctx):
    """the vgg16 / m7 configuration: TorchvisionResize of 27 x 41 sources to 32 x 32, image and (truncated) label; with no crop
    and with a top-left crop -- and a source that has the size already"""
    rng = np.random.default_rng(8)
    S = 32
    images = [rng.integers(0, 256, (27, 41, 3)).astype(np.uint8) for _ in range(2)] + [rng.integers(0, 256, (32, 32, 3)).astype(np.uint8)]
    labels = [_labels_for(rng, 27, 41) for _ in range(2)] + [_labels_for(rng, 32, 32)]
    params = np.array([(32, 32, 0, 0, 0, 0, 0, 32, 32), (32, 32, 1, 0, 0, 0, 0, 32, 32), (32, 32, 1, 0, 0, 0, 0, 32, 32)], np.int32)
    _check_batch(ctx, images, labels, params, S, VOC_FLOAT, True, 2)
    # a top-left crop of a larger TorchvisionResize target (S = 32 from 40 x 48) and of a smaller one (24 x 20)
    params = np.array([(40, 48, 0, 0, 0, 0, 0, 32, 32), (24, 20, 1, 0, 0, 0, 0, 24, 20), (32, 32, 0, 0, 0, 0, 0, 32, 32)], np.int32)
    x, label, _ = _check_batch(ctx, images, labels, params, S, VOC_INT, False, 2)
    assert len(set(np.unique(label[0]))) > 5  # the truncated bilinear label takes values between the classes


def test_train_batch_stage0_and_no_crop(ctx):
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, (32, 32, 3)).astype(np.uint8), rng.integers(0, 256, (20, 45, 3)).astype(np.uint8)]
    labels = [_labels_for(rng, 32, 32), _labels_for(rng, 20, 45)]
    params = np.array([(32, 32, 1, 0, 0, 0, 0, 32, 32), (20, 45, 0, 12, 0, 0, 13, 20, 32)], np.int32)
    _check_batch(ctx, images, labels, params, 32, VOC_INT, False, 0)


def test_rejections_without_a_launch(ctx):
    rng = np.random.default_rng(10)
    images = [rng.integers(0, 256, (20, 25, 3)).astype(np.uint8), rng.integers(0, 256, (50, 60, 3)).astype(np.uint8)]
    labels = [_labels_for(rng, 20, 25), _labels_for(rng, 50, 60)]
    good = [(24, 30, 0, 5, 2, 0, 0, 24, 30), (45, 54, 1, 0, 0, 9, 17, 32, 32)]
    bad = {
        "window below the image": (1, (45, 54, 1, 0, 0, 14, 17, 32, 32)),
        "window right of the image": (1, (45, 54, 1, 0, 0, 9, 23, 32, 32)),
        "window outside the container": (0, (24, 30, 0, 9, 2, 0, 0, 24, 30)),
        "negative offset": (0, (24, 30, 0, 5, -1, 0, 0, 24, 30)),
    }
    for what, (b, rec) in bad.items():
        params = list(good)
        params[b] = rec
        msg = _run_batch(ctx, images, labels, params, 32, VOC_INT, False, 1, expect_error=True)
        assert "sample %d" % b in msg, (what, msg)
    msg = _run_batch(ctx, images, labels, good, 32, VOC_INT, False, 0, expect_error=True)  # stage 0 on a wrong-sized sample
    assert "sample 0" in msg and "stage 0" in msg
    src, out = Guarded(ctx, images[0].size, images[0]), Guarded(ctx, 19 * 27 * 3)
    try:
        with pytest.raises(_lib.WscError) as ei:  # order 2
            _lib.pil_resize_u8(ctx, src.ptr, [(20, 25)], np.array([0]), [(19, 27)], np.array([0]), 3, 2, out.ptr)
        assert ei.value.status == _lib.WSC_ERR_INVALID
        ctx.sync()
        assert (out.payload("resize result") == SENTINEL).all()
    finally:
        src.free()
        out.free()


# ---- TrainBatcher -> IrnTrainer.step ----------------------------------------------------------------------------------------------------
def _fresh_model(sd, ctx, S=64):
    m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=S, stride=4)
    m._ctx = ctx
    m.load_state_dict(sd)
    m.eval().cuda(0)
    return m


def test_batcher_feeds_the_trainer(ctx, tmp_path):
    """two steps of IrnTrainer fed by TrainBatcher.apply == two steps fed by the host datasets' arrays for the same records: the
    inputs are bit-equal, so the ten loss values are too"""
    import random

    S, B = 64, 2
    ds, data = synthetic_dataset(tmp_path, "voc12", rescale=(0.5, 1.5), crop_method="random", S=S, norm_mode="float",
                                 sizes=[(70, 90), (100, 60), (64, 64), (50, 130)])
    random.seed(21)
    records = [[ds.draw(i, data[i][0].shape[:2]) for i in idxs] for idxs in ((0, 1), (2, 3))]
    sd = synth.irn_state_dict("resnet50", seed=1)
    batcher = irn_train.TrainBatcher(ctx, S, "float")
    a, b = _fresh_model(sd, ctx), _fresh_model(sd, ctx)
    try:
        with irn_train.IrnTrainer(a, PathIndex(5), 0.01, 1e-4, 4) as ta, irn_train.IrnTrainer(b, PathIndex(5), 0.01, 1e-4, 4) as tb:
            for idxs, recs in zip(((0, 1), (2, 3)), records):
                items = [ds.item(i, r) for i, r in zip(idxs, recs)]
                x, label, reduced = batcher.apply([data[i][0] for i in idxs], [data[i][1] for i in idxs], np.stack(recs))
                with x, label, reduced:
                    assert x.shape == (B, 3, S, S) and label.shape == (B, S, S) and reduced.shape == (B, 16, 16)
                    assert np.array_equal(x.to_host().view(np.uint32), np.stack([it["img"] for it in items]).view(np.uint32))
                    assert np.array_equal(reduced.to_host(), np.stack([it["reduced_label"] for it in items]))
                    got = ta.step(x, reduced)
                want = tb.step(np.stack([it["img"] for it in items]), np.stack([it["reduced_label"] for it in items]))
                assert set(got) == set(_lib.IRN_LOSS_SLOTS) and got == want, (got, want)
                assert np.isfinite(got["total"]) and got["n_bg"] + got["n_fg"] + got["n_neg"] > 0
    finally:
        a._release_net()
        b._release_net()
    with pytest.raises(ValueError):
        irn_train.TrainBatcher(ctx, S, "int", outsize=(64, 64), rescale=(0.5, 1.5))


def test_train_irn_run(ctx, tmp_path, capsys):
    from wsscam.step import train_irn

    S = 64
    ds, data = synthetic_dataset(tmp_path, "voc12", sizes=[(70, 90), (100, 60), (64, 64), (50, 130)])
    sd = synth.irn_state_dict("resnet50", seed=2)
    out = str(tmp_path / "irn_weights.npy")
    lst = str(tmp_path / "train.txt")
    args = types.SimpleNamespace(
        irn_network="net.resnet50_irn", model_dir=None, dataset="voc12", tag="", num_classes=20, use_cls=None, irn_crop_size=S,
        irn_batch_size=2, irn_num_epoches=1, irn_learning_rate=0.01, irn_weight_decay=1e-4, train_list=lst, infer_list=lst,
        ir_label_out_dir=str(tmp_path / "ir_label"), dev_root=str(tmp_path), crop_method="random", rescale_range=(0.5, 1.5), outsize=None,
        norm_mode="float", irn_weights_name=out, num_workers=2, state_dict=sd, seed=0, irn_path_radius=5)
    trained = train_irn.run(args)
    own = trained.ctx  # (run's model made a context of its own)
    trained._release_net()
    own.close()
    printed = capsys.readouterr().out
    assert "Epoch 1/1" in printed and "step:    0/    2" in printed and "done." in printed
    m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=S, stride=4)
    m._ctx = ctx
    tr = irn_train.IrnTrainer.load(out, m, PathIndex(5), 0.01, 1e-4, 2)
    try:
        assert tr.global_step == 2
        got = tr.state_dict()
        assert set(got) == set(sd)
        shift = got["mean_shift.running_mean"]
        assert shift.shape == (2,) and np.isfinite(shift).all()
        heads = [k for k in sd if k.startswith("fc_")]
        assert heads and all(not np.array_equal(got[k], sd[k]) for k in heads if k.endswith(".weight"))
        assert all(np.array_equal(got[k], sd[k]) for k in sd if not k.startswith("fc_") and k != "mean_shift.running_mean")
    finally:
        tr.close()
        m._release_net()
