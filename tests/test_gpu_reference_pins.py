"""GPU: the device entry points against what the REFERENCE's own functions returned (tests/golden/ref_*.npz, written by
oracle/gen_golden_ref.py; tests/test_reference_pins.py holds the restated oracles to the same files on the CPU).  Nothing here
reads anything but those fixtures.

  wsc_cue_seeds                 labels equal on every pixel outside the oracle's `ambiguous` mask (equal-area ties, painted in
                                np.argsort's unspecified order; at most 10 % of a case, asserted -- the hand-made equal-areas case
                                IS one tie, 4 of its 16 pixels); areas equal the oracle's (the reference returns none)
  wsc_roc_thresholds            thresholds exact where status == 0; status != 0 exactly where the reference's rates are not finite
  wsc_cls_threshold_counts      the five counts exact (the reference's ratios times their integer denominators), and the ratios
                                formed from them equal the reference's to the bit
  wsc_dsrg_seed_grow            the new cue exact
  wsc_irn_aff_loss              every loss value within irn_loss_ref.loss_bound of the float64 reductions (step/train_irn.py:114-125)
                                of the reference's float64 per-pair tensors; the three pair counts exact
  wsc_hsn_background            1e-12, the bound of test_gpu_hsn.py::test_hsn_background_vs_scipy
  wsc_hsn_cs_gradcam            2e-6 (stack) and 4e-6 (margin map, where the two largest channels are tied or more than 1e-5
                                apart), the bounds of test_gpu_hsn.py, against the reference's float64 chain; the distance to its
                                float32 chain is printed beside them
  wsc_msf_input_u8              bit for bit on its equal-size path

Every output buffer lies between two bands of GUARD canary bytes and starts filled with 0xff (a NaN, label 255, count -1)."""
import json

import numpy as np
import pytest

from oracle import gen_golden_ref as gen
from oracle import hsn_ref
from tests import cls_head_ref, cue_seeds_ref, irn_loss_ref
from wsscam import _lib
from wsscam.hsn import utilities as hsn
from wsscam.misc.indexing import PathIndex
from wsscam.secdsrg import DeviceMaps

pytestmark = pytest.mark.gpu

GUARD = 1024  # canary bytes on either side of every output
CANARY, FILL = 0xA5, 0xFF
FIX = {piece: gen.load(piece) for piece in gen.PIECES}


class Out:
    """an output array on the device between two canary bands; read() checks the bands and returns the array"""

    def __init__(self, ctx, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.pad = -self.n % 256
        host = np.full(GUARD + self.n + self.pad + GUARD, CANARY, np.uint8)
        host[GUARD:GUARD + self.n] = FILL
        self.dev = DeviceMaps.from_host(ctx, host)
        self.ptr = self.dev.ptr + GUARD

    def read(self):
        raw = self.dev.to_host()
        assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + self.n:] == CANARY).all(), "a write outside the output"
        return raw[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dev.free()


def _up(ctx, a):
    return DeviceMaps.from_host(ctx, np.ascontiguousarray(a))


# ---- cue seeds --------------------------------------------------------------------------------------------------------------
def _seeds(ctx, fg, bg, per_image_max):
    B, C, H, W = fg.shape
    L = C + (bg is not None)
    with _up(ctx, fg) as f, Out(ctx, (B, H, W), np.uint8) as lab, Out(ctx, (B, L), np.int32) as area:
        b = None if bg is None else _up(ctx, bg)
        try:
            _lib.cue_seeds(ctx, f.ptr, None if b is None else b.ptr, B, C, 0 if bg is None else bg.shape[1], H, W, gen.CUE_THRESH,
                           lab.ptr, area.ptr, per_image_max=per_image_max, bg_fraction=cue_seeds_ref.BG_FRACTION)
            return lab.read(), area.read()
        finally:
            if b is not None:
                b.free()


@pytest.mark.parametrize("name", gen.cases_of(FIX["cue_seeds"]))
def test_cue_seeds_equal_the_reference(ctx, name):
    d = FIX["cue_seeds"]
    fg, bg = d[name + "/fg"], d.get(name + "/bg")
    for key, use_bg, per_image in (("labels_batch", bg, False), ("labels_image", None, True)):
        want = d[name + "/" + key]
        _, want_area, amb = cue_seeds_ref.seeds(fg, use_bg, gen.CUE_THRESH, per_image_max=per_image)
        assert gen.ambiguous_ok(name, float(amb.mean())), (name, key, float(amb.mean()))
        lab, area = _seeds(ctx, fg, use_bg, per_image)
        print("cue_seeds %s %s: %d pixels compared, %d left out" % (name, key, (~amb).sum(), amb.sum()))
        assert np.array_equal(lab[~amb], want[~amb]), (name, key, int((lab != want)[~amb].sum()))
        assert np.array_equal(area, want_area), (name, key)


# ---- ROC --------------------------------------------------------------------------------------------------------------------
def _counts_of_the_reference(d, name):
    """the five counts behind the reference's ratios: each ratio times its integer denominator is within 1e-9 of an integer"""
    targets = d[name + "/targets"]
    N = len(targets)
    P, Nn = (targets == 1).sum(0), (targets == 0).sum(0)
    tpr, fpr, _, _, acc, _ = d[name + "/class_metrics"]

    def whole(x):
        r = np.rint(x)
        assert np.abs(x - r).max() < 1e-9
        return r.astype(np.int64)

    tp = whole(np.where(P > 0, tpr, 0) * P)
    fp = whole(np.where(Nn > 0, fpr, 0) * Nn)
    return np.stack([tp, fp, Nn - fp, P - tp, whole(acc * N)], axis=1)


@pytest.mark.parametrize("name", gen.cases_of(FIX["roc"]))
def test_roc_thresholds_and_counts_equal_the_reference(ctx, name):
    d = FIX["roc"]
    scores, targets, want_thr, finite = d[name + "/scores"], d[name + "/targets"], d[name + "/thresholds"], d[name + "/rates_finite"]
    N, C = scores.shape
    with _up(ctx, scores) as sd, _up(ctx, targets) as td, _up(ctx, want_thr) as ref_thr, Out(ctx, (C,), np.float32) as thr, \
            Out(ctx, (C,), np.int32) as status, Out(ctx, (C,), np.int32) as n_points, Out(ctx, (C, N + 1), np.int32) as fps, \
            Out(ctx, (C, N + 1), np.int32) as tps, Out(ctx, (C, 5), np.int64) as counts:
        _lib.roc_thresholds(ctx, sd.ptr, td.ptr, N, C, thr.ptr, status.ptr, n_points_dev=n_points.ptr, fps_dev=fps.ptr, tps_dev=tps.ptr)
        _lib.cls_threshold_counts(ctx, sd.ptr, td.ptr, N, C, ref_thr.ptr, counts.ptr)  # at the REFERENCE's thresholds (+inf included)
        got_thr, got_status, got_n, got_fps, got_tps, got_counts = (o.read() for o in (thr, status, n_points, fps, tps, counts))
    assert np.array_equal(got_status != 0, ~finite), (name, got_status, finite)
    ok = got_status == 0
    assert np.array_equal(got_thr[ok], want_thr[ok]), (name, got_thr, want_thr)
    assert np.array_equal(got_n[ok], d[name + "/n_points"][ok])
    for c in np.nonzero(ok)[0]:  # the kept curve is the reference's
        K = got_n[c]
        assert np.array_equal(got_fps[c, :K] / np.float64(got_fps[c, K - 1]), d[name + "/fprs"][c, :K]), (name, c)
        assert np.array_equal(got_tps[c, :K] / np.float64(got_tps[c, K - 1]), d[name + "/tprs"][c, :K]), (name, c)
    assert np.array_equal(got_counts, _counts_of_the_reference(d, name)), name
    per_class, overall = gen.count_ratios(got_counts, N)
    assert np.array_equal(per_class, d[name + "/class_metrics"], equal_nan=True)
    assert np.array_equal(overall, d[name + "/overall_metrics"], equal_nan=True)
    print("roc %s: %d of %d thresholds compared, %d classes without positives or negatives" % (name, ok.sum(), C, (~ok).sum()))


# ---- DSRG -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gen.cases_of(FIX["dsrg"]))
def test_dsrg_seed_grow_equals_the_reference(ctx, name):
    d = FIX["dsrg"]
    tags, cues, probs, want = d[name + "/tags"], d[name + "/cues"], d[name + "/probs"], d[name + "/new_cues"]
    B, H, W, C = cues.shape
    with _up(ctx, tags) as t, _up(ctx, cues) as c, _up(ctx, probs) as p, Out(ctx, cues.shape, np.float32) as out:
        _lib.dsrg_seed_grow(ctx, t.ptr, c.ptr, p.ptr, B, H, W, C, out.ptr)
        got = out.read()
        assert np.array_equal(c.to_host(), cues)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


# ---- IRNet loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gen.cases_of(FIX["irn_loss"]))
def test_irn_aff_loss_equals_the_reference(ctx, name):
    d = FIX["irn_loss"]
    edge, dp, label, radius = d[name + "/edge"], d[name + "/dp"], d[name + "/label"], int(d[name + "/radius"])
    B, h, w = edge.shape
    pi = PathIndex(radius)
    dirs, start, yx = pi.device_tables()
    n_slots = len(irn_loss_ref.KEYS)
    with _up(ctx, edge) as e, _up(ctx, dp) as q, _up(ctx, label) as lab, Out(ctx, (n_slots,), np.float64) as loss, \
            Out(ctx, (B, h, w), np.float32) as ge, Out(ctx, (B, 2, h, w), np.float32) as gd:
        _lib.irn_aff_loss(ctx, e.ptr, q.ptr, lab.ptr, B, h, w, dirs, start, yx, pi.radius_floor, 21, loss.ptr,
                          grad_edge_dev=ge.ptr, grad_dp_dev=gd.ptr)
        got, g_e, g_d = loss.read(), ge.read(), gd.read()
    assert np.isfinite(g_e).all() and np.isfinite(g_d).all()
    want, mag, terms = gen.irn_reductions(d, name, "f64")
    want32, _, _ = gen.irn_reductions(d, name, "f32")
    worst = to32 = 0.0
    for k, key in enumerate(irn_loss_ref.KEYS):
        if key.startswith("n_"):
            assert got[k] == want[key], (name, key, got[k], want[key])
            continue
        err = abs(got[k] - want[key])
        worst, to32 = max(worst, err / mag[key]), max(to32, abs(got[k] - want32[key]) / mag[key])
        assert err <= irn_loss_ref.loss_bound(mag[key], terms[key]), (name, key, got[k], want[key], mag[key])
    print("irn_aff_loss %s: pairs %d / %d / %d; max |err| / sum|terms| %.3g to the reference's float64 tensors, %.3g to its float32 ones"
          % (name, got[7], got[8], got[9], worst, to32))


# ---- HistoSegNet ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hsn_background(ctx):
    """wsc_hsn_background of the fixture's images: float64 (B, S, S), computed once"""
    img = FIX["hsn"]["b2/images"]
    B, S = img.shape[:2]
    with _up(ctx, img) as rgb, Out(ctx, (B, S, S), np.float64) as bg:
        _lib.hsn_background(ctx, rgb.ptr, B, S, S, bg.ptr)
        return bg.read()


def _valid_stack(H, htt):
    classes, inds = hsn_ref.adp_class_tables()
    Y = np.zeros((H.shape[0], len(classes["valid_" + htt])) + H.shape[2:])
    Y[:, inds[htt + "2valid"]] = H[:, inds["all2" + htt]]
    return Y, classes, inds


def test_hsn_background_equals_the_reference(hsn_background):
    d = FIX["hsn"]
    Y0, classes, _ = _valid_stack(d["b2/H"], "morph")
    _, _, ex = hsn._htt_tables(classes["valid_morph"], False)
    # the reference returns the background minus the strongest exception class: the same subtraction on the device's background
    got = hsn_background - Y0[:, ex].max(axis=1)
    err = np.abs(got - d["b2/Y_morph_f64"][:, 0]).max()
    err32 = np.abs(got - d["b2/Y_morph_f32"][:, 0]).max()
    print("hsn_background: max |err| %.3g to the reference's float64 chain (bound 1e-12), %.3g to its float32 chain" % (err, err32))
    assert hsn_background.max() > 0.5  # the bright regions are there
    assert err <= 1e-12


@pytest.mark.parametrize("htt", ["morph", "func"])
def test_hsn_cs_gradcam_equals_the_reference(ctx, hsn_background, htt):
    d = FIX["hsn"]
    H = d["b2/H"]
    B, C_all, S, _ = H.shape
    N = S * S
    _, classes, inds = _valid_stack(H, htt)
    valid = classes["valid_" + htt]
    Cv = len(valid)
    src_of = [-1] * Cv
    for v, a in zip(inds[htt + "2valid"], inds["all2" + htt]):
        src_of[v] = a
    morph_src = dict(zip(inds["morph2valid"], inds["all2morph"]))
    adipose_src = [morph_src[v] for v in gen.HSN_ADIPOSE_VALID] if htt == "func" else None  # (none of them is channel 0)
    bg_ind, other_ind, ex = hsn._htt_tables(valid, htt == "func")
    with _up(ctx, H.reshape(B, C_all, N)) as Hd, _up(ctx, hsn_background) as bg, Out(ctx, (B, Cv, S, S), np.float32) as cs, \
            Out(ctx, (B, Cv, S, S), np.float32) as y, Out(ctx, (B, Cv), np.uint32) as mass:
        _lib.hsn_cs_gradcam(ctx, Hd.ptr, B, C_all, N, bg.ptr, src_of, bg_ind, other_ind, ex, adipose_src, cs.ptr, y.ptr, mass.ptr)
        got_cs, got_y, got_mass = cs.read(), y.read(), mass.read()
    Y64, Y32, cs64, cs32 = (d["b2/%s_%s_%s" % (a, htt, t)] for a in ("Y", "cs") for t in ("f64", "f32"))
    safe = np.broadcast_to(gen.hsn_safe(Y64)[:, None], got_cs.shape)
    err_y, err_cs = np.abs(got_y - Y64).max(), np.abs(got_cs - cs64)[safe].max()
    print("hsn_cs_gradcam %s: stack max |err| %.3g to the float64 chain (bound 2e-6), %.3g to the float32 chain; margin map %.3g "
          "(bound 4e-6), %.3g; %d of %d pixels compared"
          % (htt, err_y, np.abs(got_y - Y32).max(), err_cs, np.abs(got_cs - cs32)[safe].max(), safe[:, 0].sum(), safe[:, 0].size))
    assert safe.mean() > 0.99
    assert err_y <= 2e-6 and err_cs <= 4e-6
    for b in range(B):
        assert list(np.nonzero(got_mass[b])[0]) == list(hsn_ref.pass_classes(cs64[b])), b


# ---- input normalisation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["int", "float"])
@pytest.mark.parametrize("loader", gen.NORM_LOADERS)
def test_msf_input_normalisation_equals_the_reference(ctx, loader, mode):
    d = FIX["normalize"]
    img = d["37x37/image"]  # the square one: S = 37 is the equal-size path, no resize
    S = img.shape[0]
    mean, std = json.loads(str(d["meta"]))["constants"]["%s_%s" % (loader, mode)]
    want = np.ascontiguousarray(np.transpose(d["37x37/%s_%s" % (loader, mode)], (2, 0, 1)))[None]
    with _up(ctx, img.reshape(-1)) as dev, Out(ctx, (1, 3, S, S), np.float32) as x, Out(ctx, (2, 3, S, S), np.float32) as pair:
        _lib.msf_input_u8(ctx, dev.ptr, [img.shape[:2]], [0], S, mean, std, x.ptr, pre_div255=mode == "float", pair=False)
        _lib.msf_input_u8(ctx, dev.ptr, [img.shape[:2]], [0], S, mean, std, pair.ptr, pre_div255=mode == "float", pair=True)
        got, got_pair = x.read(), pair.read()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (loader, mode, np.abs(got - want).max())
    assert np.array_equal(got_pair.view(np.uint32), np.stack([want[0], np.flip(want[0], -1)]).view(np.uint32))
