"""The checkpoint files of the three trainers, pinned: every key of the saved dictionary (nested ones included) with its dtype and
shape, and the scalar entries of "__step__" by name and Python type, must stay what tests/golden/train_checkpoints.json recorded --
a file written by one commit has to load at the next and the other way round.  One small trainer of each kind (the thin nets of the
*_sgd tests), one step, one save.

The fixture is NOT made from the code under test.  It was written by hand, on the GPU, with the library of commit 44ad860 -- the
commit before the parameter codec and the trainer core got their single owners -- from the repository root:
    PYTHONPATH=.:wsss-analysis_amd python -c "from tests import test_gpu_train_checkpoints as t; t.generate()"
Run that again only when the file format is meant to change."""
import json
import os

import numpy as np
import pytest

from tests import test_gpu_cls_sgd as cls_sgd
from tests import test_gpu_irn_sgd as irn_sgd
from tests import test_gpu_seg_sgd as seg_sgd
from wsscam import _lib, cls_train, irn_train, secdsrg
from wsscam.misc.indexing import PathIndex

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_checkpoints.json")
KINDS = ["seg", "irn", "cls"]


def manifest(v):
    """a saved value -> dicts by key, arrays as ["ndarray", dtype, shape], everything else as ["scalar", its Python type]"""
    if isinstance(v, dict):
        return {str(k): manifest(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return ["ndarray", v.dtype.str, list(v.shape)]
    return ["scalar", type(v).__name__]


def save_one(ctx, kind, path):
    """a trainer of `kind` after one step (the momentum is not all zeros), saved to `path`"""
    if kind == "seg":
        weights, x, cues, tags = seg_sgd._step_case("DSRG")
        tr = secdsrg.SegTrainer("DSRG", weights, 5, ctx=ctx)
        try:
            seg_sgd._trainer_step(tr, x, cues, tags, epoch=0)
            tr.save(path)
        finally:
            tr.close()
        return
    if kind == "irn":
        m = irn_sgd.fresh_model("vgg16", irn_sgd.base_sd("vgg16"), ctx=ctx)
        tr = irn_train.IrnTrainer(m, PathIndex(5), irn_sgd.LR, irn_sgd.WD, irn_sgd.MAX_STEP, power=irn_sgd.POWER)
        step = lambda: tr.step(*irn_sgd._trainer_case())  # noqa: E731
    else:
        m = cls_sgd.fresh_model("m7-keras", cls_sgd.base_sd("m7-keras"), _lib.PREC_F16X3, ctx=ctx)
        tr = cls_train.ClsTrainer(m, "max", cls_sgd.C, drop_prob=0.5, seed=3)  # (dropout on: seed and drop_prob travel in "__step__")
        x, targets, sw = cls_sgd._trainer_case()
        step = lambda: tr.step(x, targets, 0.01, sw)  # noqa: E731
    try:
        step()
        tr.save(path)
    finally:
        tr.close()
        m._release_net()


def saved_manifest(ctx, kind, path):
    save_one(ctx, kind, path)
    return manifest(np.load(path, allow_pickle=True).item())


def generate(tmp_dir="."):
    """(by hand, see the module docstring) writes the fixture from the library this tree has built"""
    ctx = _lib.Context(0)
    out = {}
    for kind in KINDS:
        path = os.path.join(tmp_dir, "_manifest_%s.npy" % kind)
        try:
            out[kind] = saved_manifest(ctx, kind, path)
        finally:
            if os.path.exists(path):
                os.remove(path)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_manifest(ctx, tmp_path, kind):
    with open(GOLDEN) as f:
        want = json.load(f)[kind]
    got = json.loads(json.dumps(saved_manifest(ctx, kind, str(tmp_path / (kind + ".npy")))))
    assert sorted(got) == sorted(want), (kind, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k] == want[k], (kind, k, got[k], want[k])
    assert all(v[0] == "scalar" for v in got["__step__"].values()), got["__step__"]
