"""GPU: Model.train on the device (secdsrg.SegTrainLoop / train, shuffled_ids, SegBatcher) on thin SEC / DSRG nets, C = 5, 65 x 65
inputs (9 x 9 maps), six PNG files, batch_size 2, two epochs of three iterations.

  composition   a second SegTrainer driven by hand with shuffled_ids, SegBatcher.train_batch and step(epoch=...) on the same
                schedule ends at final-0.npy's params, momentum and accumulator, BIT FOR BIT; the reports hold the means of its
                losses, the rate and the epoch
  resume        max_epochs = 1, then max_epochs = 2 on the same save_dir: final-0.npy equals the uninterrupted run's bits
  validation    the reported mIoU equals seg_metrics_from_confusion of a host count (np.argmax of rescale_output_dev, val_batch_host's
                ground truth, np.bincount)
  errors        no batch at all is a ValueError before anything is created; a cue entry outside the plane raises, names the
                sample and leaves the trainer as it was"""
import os

import numpy as np
import pytest
from PIL import Image

from tests import deeplab_ref as ref
from wsscam import _lib, secdsrg

pytestmark = pytest.mark.gpu

CRF_CFG = {"g_sxy": 3, "g_compat": 3, "bi_sxy": 80, "bi_srgb": 13, "bi_compat": 10, "iterations": 2}
MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)
C, SIZE, SEED_SIZE, BS, PER_EPOCH, SEED = 5, (65, 65), 9, 2, 3, 5
BASE_LR = 1e-6  # (a rate at which the thin random nets keep a softmax that is no one-hot row)
IMAGE_HW = ((20, 17), (31, 40), (24, 24), (29, 18), (21, 37), (30, 33))
CASES = [("DSRG", 1, 0.0), ("DSRG", 2, 0.5), ("SEC", 1, 0.0), ("SEC", 2, 0.0)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """six RGB PNGs, their ground-truth PNGs (class indices 0..4 and 255) and random cue lists at the map's size"""
    root = tmp_path_factory.mktemp("seg_train_loop")
    rng = np.random.default_rng(11)
    ids, cues = ["img%d" % k for k in range(len(IMAGE_HW))], {}
    for i, (h, w) in zip(ids, IMAGE_HW):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(root / (i + ".png")))
        Image.fromarray(np.array([0, 1, 2, 3, 4, 255], np.uint8)[rng.integers(0, 6, (h, w))]).save(str(root / (i + "_gt.png")))
        n = int(rng.integers(5, 40))
        cues[i + "_cues"] = np.stack([rng.integers(0, C, n), rng.integers(0, SEED_SIZE, n), rng.integers(0, SEED_SIZE, n)])
        cues[i + "_labels"] = np.unique(cues[i + "_cues"][0])
    load_image = lambda i: np.asarray(Image.open(str(root / (i + ".png"))).convert("RGB"))
    load_gt = lambda i: np.asarray(Image.open(str(root / (i + "_gt.png"))))
    return ids, cues, load_image, load_gt


def _kwargs(ctx, accum_num, drop_prob, **more):
    kw = dict(batch_size=BS, max_epochs=2, accum_num=accum_num, drop_prob=drop_prob, seed=SEED, img_mean=MEAN, crf_config_train=CRF_CFG,
              size=SIZE, seed_size=SEED_SIZE, report_every=2, ctx=ctx, num_workers=2, base_lr=BASE_LR)
    kw.update(more)
    return kw


def _weights(method):
    return ref.thin_case(method, C, SIZE)[0]


def _flat_state(net, path):
    """params, momentum and accumulator of a checkpoint file, flat in the trainer's layout"""
    d = np.load(path, allow_pickle=True).item()
    layers = {k: v for k, v in d.items() if not k.startswith("__")}
    return [net.flat_params(w) for w in (layers, d["__momentum__"], d["__accum__"])], d["__step__"]


@pytest.fixture(scope="module")
def full_runs(ctx, data, tmp_path_factory):
    """the uninterrupted two-epoch run of a case, made once: case -> (reports, save_dir)"""
    done = {}

    def run(case):
        if case not in done:
            method, accum_num, drop_prob = case
            ids, cues, load_image, _ = data
            save_dir = str(tmp_path_factory.mktemp("full_%s_%d" % (method, accum_num)))
            done[case] = (secdsrg.train(method, _weights(method), C, ids, load_image, cues, save_dir=save_dir,
                                        **_kwargs(ctx, accum_num, drop_prob)), save_dir)
        return done[case]

    return run


@pytest.mark.parametrize("case", CASES, ids=["%s-accum%d-drop%g" % c for c in CASES])
def test_loop_is_the_composition(ctx, data, full_runs, case):
    method, accum_num, drop_prob = case
    ids, cues, load_image, _ = data
    reports, save_dir = full_runs(case)
    assert sorted(os.listdir(save_dir)) == ["epoch-3.npy", "epoch-6.npy", "final-0.npy"]
    tr = secdsrg.SegTrainer(method, _weights(method), C, ctx=ctx, accum_num=accum_num, drop_prob=drop_prob, seed=SEED, base_lr=BASE_LR)
    try:
        batcher = secdsrg.SegBatcher(C, MEAN, size=SIZE, seed_size=SEED_SIZE, ctx=ctx)
        order = secdsrg.shuffled_ids(len(ids), SEED)
        steps = []
        for i in range(2 * PER_EPOCH):
            batch = [ids[next(order)] for _ in range(BS)]
            x, cu, lab = batcher.train_batch(batch, [load_image(k) for k in batch], cues)
            with x, cu, lab:
                losses, new_cues = tr.step(x, cu, lab, MEAN, CRF_CFG, epoch=i / PER_EPOCH if i % PER_EPOCH == 0 else None)
                if new_cues is not cu:
                    new_cues.free()
            steps.append((losses, float(tr.lr)))
        (params, mom, accum), step = _flat_state(tr.net, os.path.join(save_dir, "final-0.npy"))
        for name, got, want in (("params", params, tr.params), ("mom", mom, tr.mom), ("accum", accum, tr.accum)):
            assert np.array_equal(_bits(got), _bits(want.to_host())), (name, int((_bits(got) != _bits(want.to_host())).sum()))
        assert step["calls"] == tr.calls == 6 and np.abs(tr.mom.to_host()).max() > 0
        assert not np.array_equal(_bits(params), _bits(tr.net.flat_params(_weights(method))))  # it did train
        # the reports: iterations 0, 2, 4, each the mean over the steps since the last one
        assert [r["iteration"] for r in reports] == [0, 2, 4] and [r["epoch"] for r in reports] == [0.0, 2 / 3, 4 / 3]
        for r, span in zip(reports, ((0,), (1, 2), (3, 4))):
            for key in ("seed", "constrain", "total"):
                assert r[key] == sum([steps[k][0][key] for k in span], 0.0) / len(span), (r["iteration"], key)
            assert r["lr"] == steps[span[-1]][1] == float(tr.lr_at(r["epoch"])) and r["miou"] == {}
            print("%s accum %d drop %g, iteration %d: seed %.6f constrain %.6f total %.6f lr %.3e"
                  % (method, accum_num, drop_prob, r["iteration"], r["seed"], r["constrain"], r["total"], r["lr"]))
    finally:
        tr.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["DSRG-accum2-drop0.5", "SEC-accum1-drop0"])
def test_resume_equals_the_uninterrupted_run(ctx, data, full_runs, case, tmp_path):
    method, accum_num, drop_prob = case
    ids, cues, load_image, _ = data
    _, full_dir = full_runs(case)
    save_dir = str(tmp_path)
    first = secdsrg.train(method, _weights(method), C, ids, load_image, cues, save_dir=save_dir, **_kwargs(ctx, accum_num, drop_prob, max_epochs=1))
    assert sorted(os.listdir(save_dir)) == ["epoch-3.npy", "final-0.npy"] and [r["iteration"] for r in first] == [0, 2]
    second = secdsrg.train(method, _weights(method), C, ids, load_image, cues, save_dir=save_dir, **_kwargs(ctx, accum_num, drop_prob))
    assert sorted(os.listdir(save_dir)) == ["epoch-3.npy", "epoch-6.npy", "final-0.npy"] and [r["iteration"] for r in second] == [4]
    net = secdsrg.SegNet(method, _weights(method), C, ctx=ctx)
    try:
        for name in ("epoch-3.npy", "epoch-6.npy", "final-0.npy"):
            got, step = _flat_state(net, os.path.join(save_dir, name))
            want, step_w = _flat_state(net, os.path.join(full_dir, name))
            assert step == step_w and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)), name
        # a checkpoint directory as the initial weights: final-0.npy's weights alone, a fresh optimiser
        with secdsrg.SegTrainLoop(method, save_dir, C, ids, load_image, cues, **_kwargs(ctx, accum_num, drop_prob)) as loop:
            assert np.array_equal(_bits(loop.trainer.params.to_host()), _bits(want[0])) and loop.i == 0 and loop.trainer.calls == 0
            assert not loop.trainer.mom.to_host().any()
    finally:
        net.close()


def test_validation_miou(ctx, data):
    ids, cues, load_image, load_gt = data
    val_ids = ids[1:4]  # two batches: 2 + 1
    # accum_num beyond the run's length: no update is applied, so the net validates -- at every report -- with the initial weights
    with secdsrg.SegTrainLoop("DSRG", _weights("DSRG"), C, ids, load_image, cues, val_sets={"val": (val_ids, load_image, load_gt)},
                              **_kwargs(ctx, 4, 0.0, max_epochs=1)) as loop:
        start = loop.trainer.params.to_host()
        reports = loop.run()
        assert np.array_equal(_bits(loop.trainer.params.to_host()), _bits(start)) and loop.trainer.calls == 3
        images, gts = [load_image(i) for i in val_ids], [load_gt(i) for i in val_ids]
        x, gt_dev = loop.batcher.val_batch(images, gts)
        with x, gt_dev:
            with loop.trainer.net.rescale_output_dev(x, MEAN, CRF_CFG, seed_size=SEED_SIZE) as out:
                pred = np.argmax(out.to_host(), axis=-1)
            gt = loop.batcher.val_batch_host(images, gts)[1]
            assert np.array_equal(gt_dev.to_host(), gt)
    conf = np.bincount(gt.reshape(-1).astype(np.int64) * (C + 1) + pred.reshape(-1), minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    want = secdsrg.seg_metrics_from_confusion(conf)["mIoU"]
    assert [r["iteration"] for r in reports] == [0, 2] and conf[C].sum() > 0
    assert reports[0]["miou"] == {"val": want} and reports[1]["miou"] == {"val": want}
    print("validation mIoU %.6f over %d pixels" % (want, conf.sum()))


def test_no_batch_is_a_value_error(ctx, data):
    ids, cues, load_image, _ = data
    with pytest.raises(ValueError, match="no batch"):
        secdsrg.train("DSRG", None, C, ids, load_image, cues, **_kwargs(ctx, 1, 0.0, batch_size=len(ids) + 1))  # (the weights are never read)


def test_a_bad_cue_names_the_sample(ctx, data):
    ids, cues, load_image, _ = data
    order = secdsrg.shuffled_ids(len(ids), SEED)
    victim = ids[[next(order) for _ in range(BS)][1]]  # the second sample of the first batch
    bad = dict(cues)
    bad[victim + "_cues"] = np.concatenate([cues[victim + "_cues"], np.array([[1], [SEED_SIZE], [0]])], axis=1)  # row == seed_size
    with secdsrg.SegTrainLoop("DSRG", _weights("DSRG"), C, ids, load_image, bad, **_kwargs(ctx, 1, 0.0)) as loop:
        start = loop.trainer.params.to_host()
        with pytest.raises(_lib.WscError, match="sample 1") as ei:
            loop.run()
        assert ei.value.status == _lib.WSC_ERR_INVALID
        assert loop.trainer.calls == 0 and np.array_equal(_bits(loop.trainer.params.to_host()), _bits(start))
