"""GPU: wsc_dsrg_seed_grow (csrc/dsrg.hip) and the 03a mirrors of wsscam.secdsrg against the numpy / scipy oracle of
tests/dsrg_ref.py.  The result is 0/1, so every comparison is np.array_equal."""
import numpy as np
import pytest

from tests import dsrg_ref, helpers
from wsscam import _lib, secdsrg

pytestmark = pytest.mark.gpu


def _grow(ctx, tags, cues, probs, in_place=False, th_f=dsrg_ref.TH_F, th_b=dsrg_ref.TH_B):
    """The raw entry point on a batch: (B, C) tags, (B, H, W, C) cues / probs -> float32 (B, H, W, C)."""
    B, H, W, C = cues.shape
    t_dev, c_dev, p_dev = (ctx.to_device(np.asarray(a, np.float32)) for a in (tags, cues, probs))
    o_dev = c_dev if in_place else ctx.alloc(cues.size * 4)
    if not in_place:
        _lib.check(ctx._lib.wsc_memset(ctx.h, o_dev.ptr, 0xff, cues.size * 4))  # every cell must be written
    _lib.dsrg_seed_grow(ctx, t_dev, c_dev, p_dev, B, H, W, C, o_dev, th_f=th_f, th_b=th_b)
    out = ctx.to_host(o_dev, (B, H, W, C), np.float32)
    if not in_place:
        assert np.array_equal(ctx.to_host(c_dev, (B, H, W, C), np.float32), cues)
    return out


@pytest.fixture(scope="module")
def sweep():
    """[(name, tags, cues, probs, oracle output, grown, blocked)], computed once."""
    return [(name, t, c, p) + dsrg_ref.seed_grow_batch(t, c, p) for name, t, c, p in dsrg_ref.sweep_cases()]


def test_sweep_is_not_vacuous(sweep):
    """A condition on the INPUTS: the oracle grows and blocks cells on them, and images of a batch differ in their tags."""
    assert sum(s[5] for s in sweep) >= 100 and sum(s[6] for s in sweep) >= 10
    tags = {s[0]: s[1] for s in sweep}["33x65x29"]
    assert not np.array_equal(tags[0], tags[1])


@pytest.mark.parametrize("idx", range(len(dsrg_ref.SWEEP)), ids=[s[0] for s in dsrg_ref.SWEEP])
def test_seed_grow_equals_oracle(ctx, sweep, idx):
    name, tags, cues, probs, ref, _, _ = sweep[idx]
    out = _grow(ctx, tags, cues, probs)
    assert out.shape == ref.shape and np.array_equal(out, ref), name
    # out_dev == cues_dev: the same array
    assert np.array_equal(_grow(ctx, tags, cues, probs, in_place=True), ref), name


@pytest.mark.parametrize("case", dsrg_ref.handmade_cases(), ids=lambda c: c[0])
def test_handmade_cases(ctx, case):
    name, tag, cue, prob, expect = case
    for in_place in (False, True):
        out = _grow(ctx, tag[None], cue[None], prob[None], in_place=in_place)
        assert np.array_equal(out[0], expect), (name, in_place)


def test_thresholds_are_arguments(ctx, sweep):
    _, tags, cues, probs, ref, _, _ = sweep[0]
    want, grown, _ = dsrg_ref.seed_grow_batch(tags, cues, probs, th_f=0.85, th_b=0.99)
    assert grown > 0 and not np.array_equal(want, ref)
    assert np.array_equal(_grow(ctx, tags, cues, probs, th_f=0.85, th_b=0.99), want)


def test_limits(ctx):
    buf = ctx.alloc(1 << 20)

    def call(B, H, W, C, tags=buf, cues=buf, probs=buf, out=buf):
        _lib.dsrg_seed_grow(ctx, tags, cues, probs, B, H, W, C, out)

    for args, word in (((1, 91, 91, 2), "8281 pixels"), ((1, 1, 8193, 2), "8193"), ((1, 8, 8, 33), "C=33"),
                       ((1, 8, 8, 0), "C=0"), ((0, 8, 8, 2), "B=0"), ((1, 0, 8, 2), "H=0"), ((1, 8, -3, 2), "W=-3")):
        with pytest.raises(_lib.WscError) as ei:
            call(*args)
        assert ei.value.status == _lib.WSC_ERR_INVALID and word in str(ei.value), (args, str(ei.value))
    for null in ("tags", "cues", "probs", "out"):
        with pytest.raises(_lib.WscError) as ei:
            call(1, 8, 8, 2, **{null: None})
        assert ei.value.status == _lib.WSC_ERR_INVALID
    # the largest image the entry point takes, at the largest class count: one component over everything
    H, W, C = 64, 128, 32
    tag = np.zeros(C, np.float32)
    tag[31] = 1
    cue = np.zeros((H, W, C), np.float32)
    cue[H - 1, W - 1, 31] = 1
    prob = np.full((H, W, C), 0.9, np.float32)
    out = _grow(ctx, tag[None], cue[None], prob[None])
    assert np.array_equal(out[0], dsrg_ref.seed_grow(tag, cue, prob)[0]) and out[0, :, :, 31].all() and out.sum() == H * W


def test_generate_seed_step(ctx, sweep):
    _, tags, cues, probs, ref, _, _ = sweep[0]
    B, H, W, C = cues.shape
    cues_in, probs_in, tags_in = cues.copy(), probs.copy(), tags.copy()
    for t in (tags_in, tags_in.reshape(B, 1, 1, C)):
        out = secdsrg.generate_seed_step(t, cues_in, probs_in, ctx=ctx)
        assert out.dtype == np.float32 and out.shape == (B, H, W, C)
        for b in range(B):
            assert np.array_equal(out[b], dsrg_ref.seed_grow(tags[b], cues[b], probs[b])[0])
        assert np.array_equal(out, ref)
        assert np.array_equal(cues_in, cues) and np.array_equal(probs_in, probs) and np.array_equal(tags_in, tags)
    # float64 inputs, as a py_func may hand them over
    assert np.array_equal(secdsrg.generate_seed_step(tags.astype(np.float64), cues.astype(np.float64), probs, ctx=ctx), ref)
    with pytest.raises(ValueError):
        secdsrg.generate_seed_step(tags[:, :-1], cues, probs, ctx=ctx)


def test_crf_layer(ctx):
    """The `crf` closure of DSRG.py:323-332 on one batched wsc_crf: marginals against the C oracle per image (the bound of
    tests/test_gpu_net.py::test_crf_inference_mirror), the log tail exactly."""
    rng = np.random.default_rng(33)
    B, H, W, C = 3, 41, 41, 5
    cfg = {"g_sxy": 3 / 12, "g_compat": 3, "bi_sxy": 80 / 12, "bi_srgb": 13, "bi_compat": 10, "iterations": 5}
    cases = [helpers.synth_crf_case(rng, H, W, C) for _ in range(B)]
    image = np.stack([rgb for rgb, _, _ in cases]).astype(np.float32)  # the py_func receives a float image (:325)
    fm = np.stack([np.transpose(p, (1, 2, 0)) for _, _, p in cases]).astype(np.float32)
    min_prob = 1e-4
    out, q = secdsrg.crf_layer(fm, image, cfg, C, min_prob=min_prob, ctx=ctx, return_q=True)
    assert out.shape == q.shape == (B, H, W, C) and out.dtype == q.dtype == np.float32
    for b in range(B):
        U = np.ascontiguousarray(-np.log(np.transpose(fm[b], (2, 0, 1)).reshape(C, -1)))
        qr, _, _ = helpers.crf_oracle(cases[b][0], U, (cfg["g_sxy"], 3, cfg["bi_sxy"], 13, 10, 5))
        assert np.abs(q[b] - np.transpose(qr.reshape(C, H, W), (1, 2, 0))).max() <= 1e-3, b
    ret = q.copy()
    ret[ret < min_prob] = min_prob
    ret /= np.sum(ret, axis=3, keepdims=True)
    ret = np.log(ret)
    assert np.array_equal(out, ret.astype(np.float32))
    assert np.abs(np.exp(out.astype(np.float64)).sum(axis=3) - 1).max() <= C * 2.0 ** -23  # one fp32 rounding per class
    assert np.array_equal(secdsrg.crf_layer(fm, image, cfg, C, min_prob=min_prob, ctx=ctx), out)
