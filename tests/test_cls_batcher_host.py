"""CPU: the host half of the 01_train generators (wsscam.cls_train.ClsBatcher, train_schedule, train, find_latest_checkpoint) -- the
order of an epoch, the drawn parameters, the state for a resume, the schedule train hands to the steps -- with the device half
(ClsBatcher.apply, ClsTrainer, the validation pass) stubbed: nothing here needs a GPU or the library."""
import os

import numpy as np
import pytest
from PIL import Image

from tests import cls_batch_ref as ref
from wsscam import cls_train


class HostBatcher(cls_train.ClsBatcher):
    """the device call replaced by the numpy restatement"""

    def apply(self, images, affine, flags):
        aug = self.augmenter
        return ref.batch(images, self.hw, affine, flags, aug.fill_mode, aug.cval, *aug.standardisation())


def _files(tmp_path, n):
    paths = []
    for i in range(n):
        img = ref.image(60 + i, (20 + i, 31 - i))
        if i == 1:  # a grey file and one with an alpha channel: load_img converts both to RGB
            im = Image.fromarray(img[:, :, 0])
        elif i == 2:
            im = Image.fromarray(np.dstack([img, img[:, :, :1]]), "RGBA")
        else:
            im = Image.fromarray(img)
        paths.append(str(tmp_path / ("im%02d.png" % i)))
        im.save(paths[-1])
    return paths


def _labels(n, C=4):
    return (np.random.RandomState(1).random_sample((n, C)) < 0.4).astype(np.float32)


def _batcher(paths, seed=3, shuffle=True, batch_size=3, cls=HostBatcher):
    return cls(paths, _labels(len(paths)), cls_train.ImageAugmenter.for_dataset("VOC2012", True), (17, 33), batch_size, shuffle, seed)


def test_every_sample_once_per_epoch_and_the_last_batch_is_short(tmp_path):
    paths = _files(tmp_path, 8)
    b = _batcher(paths)
    assert (b.n, len(b), b.data.shape, b.data.dtype) == (8, 3, (8, 4), np.float32)
    assert np.array_equal(b.data.sum(axis=0), _labels(8).sum(axis=0))
    for epoch in range(3):
        plans = [b.plan() for _ in range(len(b))]
        assert [len(p[0]) for p in plans] == [3, 3, 2]
        assert sorted(np.concatenate([p[0] for p in plans]).tolist()) == list(range(8))
        assert b.epoch == epoch
        for idx, affine, flags in plans:
            assert affine.shape == (len(idx), 6) and affine.dtype == np.float64 and flags.shape == (len(idx),) and flags.dtype == np.int32
            assert (flags & 1).all() and not (flags & ~3).any()  # VOC: every draw warps, columns may flip, rows never
    plain = _batcher(paths, shuffle=False)
    assert np.concatenate([plain.plan()[0] for _ in range(3)]).tolist() == list(range(8))


def test_same_seed_same_order_and_parameters(tmp_path):
    paths = _files(tmp_path, 8)
    a, b, c = _batcher(paths, 3), _batcher(paths, 3), _batcher(paths, 4)
    differs = False
    for _ in range(7):
        pa, pb, pc = a.plan(), b.plan(), c.plan()
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(pa, pb))
        differs = differs or not np.array_equal(pa[0], pc[0]) or not np.array_equal(pa[1], pc[1])
    assert differs
    np.random.seed(0)
    before = np.random.get_state()[1].copy()
    a.plan()
    assert np.array_equal(np.random.get_state()[1], before)  # the global generator is not used


def test_set_state_continues_identically(tmp_path):
    paths = _files(tmp_path, 8)
    a = _batcher(paths)
    for _ in range(4):  # into the second epoch
        a.plan()
    saved = a.state()
    want = [a.plan() for _ in range(6)]
    b = _batcher(paths, seed=99)
    b.set_state(saved)
    got = [b.plan() for _ in range(6)]
    for g, w in zip(got, want):
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(g, w))
    assert (b.epoch, b.pos) == (a.epoch, a.pos)
    fresh = _batcher(paths)
    fresh.set_state(_batcher(paths).state())  # the state before the first batch
    assert np.array_equal(fresh.plan()[0], _batcher(paths).plan()[0])


def test_batches_decode_to_rgb_and_equal_the_restatement(tmp_path):
    paths = _files(tmp_path, 4)
    b = _batcher(paths, shuffle=False, batch_size=4)
    images = b.decode(range(4))
    assert [i.shape for i in images] == [(20, 31, 3), (21, 30, 3), (22, 29, 3), (23, 28, 3)] and all(i.dtype == np.uint8 for i in images)
    assert np.array_equal(images[0], ref.image(60, (20, 31)))
    assert np.array_equal(images[1], np.repeat(ref.image(61, (21, 30))[:, :, :1], 3, 2))  # grey -> R = G = B
    assert np.array_equal(images[2], ref.image(62, (22, 29)))  # the alpha channel is dropped
    twin = _batcher(paths, shuffle=False, batch_size=4)
    x, labels = next(b)
    idx, affine, flags = twin.plan()
    assert x.shape == (4, 3, 17, 33) and np.array_equal(labels, _labels(4))
    sub, div, mul = ref.STANDARDISE["VOC2012"]
    assert np.array_equal(x.view(np.uint32), ref.batch(images, (17, 33), affine, flags, "reflect", 0.0, sub, div, mul).view(np.uint32))


# ---- the schedule train hands to the steps ------------------------------------------------------------------------------------------
class FakeTrainer:
    """records what train does to a trainer"""
    log = None

    def __init__(self, model, pool, num_classes, momentum=0.9, nesterov=True):
        self.ctx, self.global_step, self.loaded_extra = None, 0, {}
        FakeTrainer.log.append(("new", pool, num_classes, momentum, nesterov))

    @classmethod
    def load(cls, path, model, pool, num_classes, **kw):
        tr = cls(model, pool, num_classes, **kw)
        d = np.load(path, allow_pickle=True).item()
        tr.global_step, tr.loaded_extra = d["__step__"], {"__train__": d["__train__"]}
        FakeTrainer.log.append(("load", os.path.basename(path)))
        return tr

    def step(self, x, targets, lr, sample_weight=None):
        assert isinstance(lr, np.float32) and sample_weight is None and len(x) == len(targets)
        FakeTrainer.log.append(("step", lr, len(targets)))
        self.global_step += 1
        return {"loss": 1.0, "binary_accuracy": 0.5, "f1": 0.25}

    def save(self, path, extra=None):
        with open(path, "wb") as fh:
            np.save(fh, dict(extra, __step__=self.global_step), allow_pickle=True)
        FakeTrainer.log.append(("save", os.path.basename(path)))

    def state_dict(self):
        return {"w": np.zeros(1, np.float32)}

    def close(self):
        FakeTrainer.log.append(("close",))


class FakeModel:
    def cuda(self):
        return self


class HostArray(np.ndarray):
    def free(self):
        pass


class FreeableBatcher(HostBatcher):
    def apply(self, images, affine, flags):
        return super().apply(images, affine, flags).view(HostArray)


@pytest.fixture
def stubbed(monkeypatch):
    FakeTrainer.log = []
    monkeypatch.setattr(cls_train, "ClsTrainer", FakeTrainer)
    monkeypatch.setattr(cls_train, "ClsBatcher", FreeableBatcher)
    monkeypatch.setattr(cls_train, "_validate", lambda model, trainer, batcher: {"val_loss": 2.0, "val_binary_accuracy": 0.5, "val_f1": 0.5})
    return FakeTrainer.log


def _train(tmp_path, paths, epochs, should_clr, **kw):
    return cls_train.train(paths, _labels(len(paths)), paths[:3], _labels(3), FakeModel(), "mean", "VOC2012_VGG16", str(tmp_path / "model"),
                           str(tmp_path / "ckpt"), epochs, 3, should_clr=should_clr, seed=5, size=17, augmenter="VOC2012", lr_dropstep=2, **kw)


def test_step_schedule_of_a_three_epoch_plan(tmp_path, stubbed):
    paths = _files(tmp_path, 8)  # n = 8, batch_size 3: steps_per_epoch = 2, and the short batch opens the next epoch
    hist = _train(tmp_path, paths, 3, False)
    steps = [e for e in stubbed if e[0] == "step"]
    assert [e[1] for e in steps] == [cls_train.step_lr(ep, 0, 1e-3, 0.5, 2) for ep in (0, 0, 1, 1, 2, 2)]
    assert [e[1] for e in steps] == [np.float32(1e-3)] * 4 + [np.float32(5e-4)] * 2
    assert [e[2] for e in steps] == [3, 3, 2, 3, 3, 2]
    assert [h["epoch"] for h in hist] == [1, 2, 3] and [h["samples"] for h in hist] == [6, 5, 5] and hist[0]["val_loss"] == 2.0
    assert hist[2]["lr"] == float(np.float32(5e-4)) and hist[0]["loss"] == 1.0
    assert [e for e in stubbed if e[0] in ("save", "load")] == [("save", "VOC2012_VGG16-02.npy")]
    assert stubbed[-1] == ("close",) and os.path.exists(str(tmp_path / "model" / "VOC2012_VGG16.npy"))


def test_cyclic_schedule_of_a_three_epoch_plan(tmp_path, stubbed):
    paths = _files(tmp_path, 8)
    _train(tmp_path, paths, 3, True)
    rates = [e[1] for e in stubbed if e[0] == "step"]
    step_size = 2 / 4 * 8 // 3  # lr_dropstep / clr_spc * n // batch_size = 1.0
    want = [cls_train.cyclic_lr(it, *cls_train.cyclic_session_rates(sess, 1e-3, 2e-2), step_size)
            for sess, it in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1))]
    assert rates == want
    assert rates[:4] == [np.float32(1e-3), np.float32(2e-2), np.float32(1e-3), np.float32(2e-2)] and rates[4:] == [np.float32(5e-4), np.float32(1e-2)]


def test_resume_continues_the_plan(tmp_path, stubbed):
    paths = _files(tmp_path, 8)
    _train(tmp_path, paths, 3, False)
    whole = [e for e in stubbed if e[0] == "step"]
    del stubbed[:]
    for name in os.listdir(str(tmp_path / "ckpt")):
        os.remove(str(tmp_path / "ckpt" / name))
    _train(tmp_path, paths, 2, False)  # stops behind its checkpoint ...
    hist = _train(tmp_path, paths, 3, False)  # ... and a second run takes it up
    assert [e for e in stubbed if e[0] in ("save", "load")] == [("save", "VOC2012_VGG16-02.npy"), ("load", "VOC2012_VGG16-02.npy")]
    assert [e for e in stubbed if e[0] == "step"] == whole and [h["epoch"] for h in hist] == [3]
    assert cls_train.find_latest_checkpoint(str(tmp_path / "ckpt"), "VOC2012_VGG16") == (str(tmp_path / "ckpt" / "VOC2012_VGG16-02.npy"), 2)
    assert cls_train.find_latest_checkpoint(str(tmp_path / "ckpt"), "VOC2012") == (None, 0)
    assert cls_train.find_latest_checkpoint(str(tmp_path / "nowhere"), "x") == (None, 0)
