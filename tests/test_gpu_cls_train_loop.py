"""GPU: cls_train.train end to end (ClsBatcher -> wsc_cls_train_batch -> ClsTrainer.step, validation, checkpoints, resume) on eight
synthetic PNG files, the small real-width VGG16-with-BatchNorm state dict of tests/cls_grad_ref.py at 33 x 33 and B = 2.

  the loop      two epochs of train leave parameters, momentum and running statistics BIT-EQUAL to a second ClsTrainer stepped by
                hand on the batches of tests/cls_batch_ref.py (the restatement pinned against PIL and scipy) at step_lr's rates;
                the per-epoch means and the validation metrics are those of the hand loop (ClsLoss.loss_step on the restated
                validation batches)
  resume        a run stopped behind its checkpoint and taken up by a second run equals the uninterrupted run to the bit
  the result    <model_dir>/<sess_id>.npy loads into a fresh model whose forward_batch scores equal the trained model's"""
import os

import numpy as np
import pytest
from PIL import Image

from tests import cls_batch_ref as ref
from tests import cls_grad_ref as gref
from tests.test_cls_batcher_host import HostBatcher
from tests.test_gpu_cls_sgd import _np_sd, fresh_model
from wsscam import _lib, cls_train
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

C, S, BATCH, SEED, SESS = 20, 33, 2, 7, "VOC2012_VGG16"
SIZES = [(40, 50), (37, 53), (50, 40), (33, 33), (44, 47), (41, 52), (36, 49), (48, 45)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_dict(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, int((_bits(got[k]) != _bits(want[k])).sum()))


def _write(folder, sizes, seed):
    os.makedirs(folder, exist_ok=True)
    paths = []
    for i, hw in enumerate(sizes):
        paths.append(os.path.join(folder, "im%02d.png" % i))
        Image.fromarray(ref.image(seed + i, hw)).save(paths[-1])
    return paths


def _train(data, model, root, epochs):
    return cls_train.train(data["paths"], data["labels"], data["val_paths"], data["val_labels"], model, "mean", SESS, os.path.join(root, "model"),
                           os.path.join(root, "ckpt"), epochs, BATCH, seed=SEED, size=S, augmenter="VOC2012", lr_dropstep=1)


def _load(root, which):
    return np.load(os.path.join(root, which), allow_pickle=True).item()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("cls_train_files"))
    rng = np.random.RandomState(2)
    return {"paths": _write(os.path.join(folder, "train"), SIZES, 500), "labels": (rng.random_sample((8, C)) < 0.3).astype(np.float32),
            "val_paths": _write(os.path.join(folder, "val"), SIZES[:3], 600), "val_labels": (rng.random_sample((3, C)) < 0.3).astype(np.float32),
            "sd": _np_sd(gref.state_dict("vgg16", True))}


@pytest.fixture(scope="module")
def whole_run(ctx, data, tmp_path_factory):
    """the uninterrupted run: two epochs -> (its folder, the history, the trained model's scores on a probe)"""
    root = str(tmp_path_factory.mktemp("cls_train_whole"))
    m = fresh_model("vgg16-bn", data["sd"], _lib.PREC_F16X3, ctx=ctx)
    try:
        hist = _train(data, m, root, 2)
        probe = np.random.default_rng(17).normal(0, 1, (1, 2, 3, S, S)).astype(np.float32)
        return root, hist, probe, m.forward_batch(probe, want_score=True)
    finally:
        m._release_net()


def test_train_is_the_hand_loop_on_the_restated_batches(ctx, data, whole_run):
    root, hist, _, _ = whole_run
    assert [h["epoch"] for h in hist] == [1, 2] and all(h["steps"] == 4 and h["samples"] == 8 for h in hist)
    m = fresh_model("vgg16-bn", data["sd"], _lib.PREC_F16X3, ctx=ctx)
    gen = HostBatcher(data["paths"], data["labels"], cls_train.ImageAugmenter.for_dataset("VOC2012", True), S, BATCH, True, SEED)
    val = HostBatcher(data["val_paths"], data["val_labels"], cls_train.ImageAugmenter.for_dataset("VOC2012", False), S, BATCH, False, SEED)
    net = m._ensure_net()
    h, F = net.cam_size(S), net.feat_channels()
    try:
        with cls_train.ClsTrainer(m, "mean", C) as tr:
            assert tr.loaded_extra == {}  # (a trainer that was not loaded from a file)
            for epoch in range(2):
                lr = cls_train.step_lr(epoch, 0, 1e-3, 0.5, 1)
                tot = {"loss": 0.0, "binary_accuracy": 0.0, "f1": 0.0}
                for _ in range(4):
                    x, t = next(gen)
                    met = tr.step(x, t, lr)
                    for k in tot:
                        tot[k] += met[k] * len(t)
                for k in tot:
                    assert hist[epoch][k] == tot[k] / 8, (epoch, k)
                assert hist[epoch]["lr"] == float(lr)
                vt, w_b = {"loss": 0.0, "binary_accuracy": 0.0, "f1": 0.0}, tr._tail_views(tr.params)
                val.reset()
                for _ in range(len(val)):
                    x, t = next(val)
                    with DeviceMaps.from_host(ctx, x) as xd, DeviceMaps(ctx, (len(t), h, h, F), np.float32) as feat:
                        net.forward_features(xd.ptr, len(t), S, feat.ptr)
                        met = tr.loss.loss_step(feat, w_b[0], w_b[1], t)
                    for k in vt:
                        vt[k] += met[k] * len(t)
                for k in vt:
                    assert hist[epoch]["val_" + k] == vt[k] / 3, (epoch, k)
                # the checkpoint behind this epoch: parameters, running statistics, momentum, the batcher
                ck = _load(root, os.path.join("ckpt", "%s-%02d.npy" % (SESS, epoch + 1)))
                _same_dict({k: v for k, v in ck.items() if not k.startswith("__")}, tr.state_dict(), "state dict %d" % epoch)
                _same_dict(ck["__momentum__"], tr.momentum_host(), "momentum %d" % epoch)
                assert ck["__step__"] == {"global_step": 4 * (epoch + 1)} and ck["__train__"]["epoch"] == epoch + 1
                assert np.array_equal(ck["__train__"]["batcher"]["order"], gen.order) and ck["__train__"]["batcher"]["pos"] == gen.pos
            assert any(np.abs(v).max() > 0 for v in tr.momentum_host().values())
            _same_dict(_load(root, os.path.join("model", SESS + ".npy")), tr.state_dict(), "the final state dict")
    finally:
        m._release_net()


def test_resumed_run_equals_the_uninterrupted_one(ctx, data, whole_run, tmp_path):
    root = whole_run[0]
    first = fresh_model("vgg16-bn", data["sd"], _lib.PREC_F16X3, ctx=ctx)
    try:
        h1 = _train(data, first, str(tmp_path), 1)  # stops behind <sess>-01.npy
    finally:
        first._release_net()
    second = fresh_model("vgg16-bn", data["sd"], _lib.PREC_F16X3, ctx=ctx)  # (its weights are replaced by the checkpoint's)
    try:
        h2 = _train(data, second, str(tmp_path), 2)
    finally:
        second._release_net()
    assert [h["epoch"] for h in h1 + h2] == [1, 2]
    for got, want in zip(h1 + h2, whole_run[1]):
        assert got == want
    for name in (os.path.join("ckpt", SESS + "-02.npy"), os.path.join("model", SESS + ".npy")):
        a, b = _load(str(tmp_path), name), _load(root, name)
        _same_dict({k: v for k, v in a.items() if not k.startswith("__")}, {k: v for k, v in b.items() if not k.startswith("__")}, name)
        if "__momentum__" in b:
            _same_dict(a["__momentum__"], b["__momentum__"], name + " momentum")
            assert a["__step__"] == b["__step__"] == {"global_step": 8}
            sa, sb = a["__train__"]["batcher"], b["__train__"]["batcher"]
            assert (sa["epoch"], sa["pos"]) == (sb["epoch"], sb["pos"]) and np.array_equal(sa["order"], sb["order"])
            assert all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(sa["rng"], sb["rng"]))


def test_final_file_loads_into_a_fresh_model(ctx, data, whole_run):
    root, _, probe, (cam, score) = whole_run
    sd = _load(root, os.path.join("model", SESS + ".npy"))
    assert not any(k.startswith("__") for k in sd)
    fresh = fresh_model("vgg16-bn", sd, _lib.PREC_F16X3, ctx=ctx)
    try:
        cam2, score2 = fresh.forward_batch(probe, want_score=True)
        assert np.array_equal(_bits(score2), _bits(score)) and np.array_equal(_bits(cam2), _bits(cam))
        untrained = fresh_model("vgg16-bn", data["sd"], _lib.PREC_F16X3, ctx=ctx)
        try:
            assert not np.array_equal(untrained.forward_batch(probe, want_score=True)[1], score)  # training moved the scores
        finally:
            untrained._release_net()
    finally:
        fresh._release_net()
