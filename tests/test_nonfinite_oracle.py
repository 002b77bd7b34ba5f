"""CPU: what tests/test_gpu_nonfinite.py takes for granted -- torch and the suite's own float64 oracles carry a NaN / inf where
the contract of DESIGN.md section 5 says the reference does, the cones of tests/nonfinite_ref.py are the cells that change, and
every placement leaves at least half of the output outside its cone with a non-finite cell inside."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cls_head_ref, irn_sgd_ref, layer_ref as lr, nonfinite_ref as nf, seg_sgd_ref
from wsscam import _lib

NAN, PINF, NINF = nf.NAN, nf.PINF, nf.NINF


def test_torch_carries_nan_and_inf():
    t = torch.tensor([NAN, PINF, NINF, -1.0, 2.0], dtype=torch.float64)
    r = torch.relu(t).numpy()
    assert np.isnan(r[0]) and r[1] == PINF and r[2] == 0.0 and r[3] == 0.0 and r[4] == 2.0  # relu(-inf) == 0: finite
    c = torch.clamp(t, 1e-7, 1.0).numpy()
    assert np.isnan(c[0]) and c[1] == 1.0 and c[2] == 1e-7  # clip keeps NaN (and bounds the infinities)
    x = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    x[0, 0, 1, 1] = NAN
    p = F.max_pool2d(x, 3, 1, 1).numpy()
    assert np.isnan(p[0, 0, :3, :3]).all() and np.isfinite(p[0, 0, 3, :]).all() and np.isfinite(p[0, 0, :, 3]).all()
    x[0, 0, 1, 1] = NINF
    assert np.isfinite(F.max_pool2d(x, 3, 1, 1).numpy()).all()  # -inf never wins a window with a number in it
    assert np.isnan(np.maximum(np.float64(NAN), 0.0)) and not np.isnan(max(0.0, NAN))  # np.maximum carries, Python's max does not


def test_torch_conv_multiplies_a_weight_by_the_padding():
    """0 * NaN = NaN: the cone of a weight is its whole output channel, border cells whose tap lies in the padding included"""
    x = torch.ones(1, 2, 5, 5, dtype=torch.float64)
    w = torch.ones(3, 2, 3, 3, dtype=torch.float64)
    w[1, 0, 0, 2] = NAN
    y = F.conv2d(x, w, padding=1).numpy()
    assert np.isnan(y[0, 1]).all() and np.isfinite(y[0, 0]).all() and np.isfinite(y[0, 2]).all()


@pytest.mark.parametrize("shape", nf.CONV_SHAPES, ids=str)
@pytest.mark.parametrize("placement", nf.CONV_PLACEMENTS)
def test_conv_cone_is_where_the_reference_changes(shape, placement):
    ops = nf.conv_operands(shape)
    cone = nf.conv_cone(shape, placement)
    clean = nf.conv_ref(ops, shape, True, False)
    assert np.isfinite(clean).all()
    # a finite change of the element moves cells of the cone and no other
    name, idx = nf.conv_place(shape, placement)
    moved = nf.conv_ref(nf.conv_poisoned(ops, shape, placement, ops[name][idx] + 3.0), shape, True, False)
    assert np.array_equal(moved[~cone], clean[~cone]) and (moved[cone] != clean[cone]).any()
    for value in nf.POISONS.values():
        for relu in (False, True):
            ref = nf.conv_ref(nf.conv_poisoned(ops, shape, placement, value), shape, True, relu)
            if relu and not nf.nonfinite(ref).any():
                assert value in (PINF, NINF)  # an infinity the ReLU cut in every cell: relu(-inf) = 0, the case pins nothing
                continue
            nf.check_placement(cone, ref)
            want = np.maximum(clean, 0) if relu else clean
            assert np.array_equal(ref[~cone], want[~cone])  # outside the cone: the clean reference, exactly
    # the finite control stays finite in float64
    assert np.isfinite(nf.conv_ref(nf.conv_poisoned(ops, shape, placement, nf.CONTROL), shape, True, True)).all()


@pytest.mark.parametrize("prec", [None, _lib.PREC_BF16])
def test_shifted_reference_is_the_computed_one(prec):
    """nonfinite_ref.conv_shifted_ref (the square-tile case's reference) against conv_ref on a 1 x 1 layer small enough for it"""
    shape = (3, 64, 21, 21, 64, 1, 1, 0)
    ops = nf.conv_operands(shape)
    if prec is not None:
        ops = dict(ops, **{n: nf.bf16_round(ops[n]) for n in ("x", "w", "residual")})
    one = {"scale": np.ones_like(ops["scale"]), "shift": np.zeros_like(ops["shift"])}
    raw = nf.conv_ref(dict(ops, **one), shape, False, False)
    for placement in nf.CONV_PLACEMENTS:
        for name, value in dict(nf.POISONS, control=nf.CONTROL).items():
            a = nf.conv_shifted_ref(ops, raw, shape, placement, value, prec)
            b = nf.conv_ref(nf.conv_poisoned(ops, shape, placement, value), shape, True, True, prec)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), (placement, name)
            fin = np.isfinite(b)
            assert (np.abs(a[fin] - b[fin]) <= 1e-12 * np.maximum(np.abs(b[fin]), 1.0) * shape[1]).all(), (placement, name)


def test_conv_cone_of_the_big_shape():
    for placement in nf.CONV_PLACEMENTS:
        cone = nf.conv_cone(nf.CONV_BIG, placement)
        assert 0 < cone.sum() and 2 * cone.sum() <= cone.size


@pytest.mark.parametrize("geom", nf.POOL_GEOMS, ids=str)
@pytest.mark.parametrize("placement", nf.POOL_PLACEMENTS)
@pytest.mark.parametrize("rule", ["torch", "same"])
def test_pool_cones(geom, placement, rule):
    H, W, stride = geom
    rng = np.random.default_rng(H * 100 + W + stride)
    x = rng.normal(0, 1, (1, H, W, 64)).astype(np.float32)
    cell = nf.pool_place(H, W, stride, placement)
    cone = nf.pool_cone(H, W, 64, 3, stride, rule, cell)
    if placement == "shared":
        assert cone.sum() >= 2  # two windows read the cell
    clean = nf.pool_ref(x, 3, stride, rule, False)
    if rule == "torch":
        assert np.array_equal(clean, lr.max_pool(x, 3, stride, 1))  # the loop and F.max_pool2d agree
    for avg in ((False, True) if rule == "same" else (False,)):
        clean = nf.pool_ref(x, 3, stride, rule, avg)
        for name, value in nf.POISONS.items():
            xp = x.copy()
            xp[(0,) + cell] = value
            ref = nf.pool_ref(xp, 3, stride, rule, avg)
            if name == "ninf" and not avg:
                assert np.isfinite(ref).all()  # (-inf loses every window: nothing to propagate, the cell is simply not the maximum)
                continue
            nf.check_placement(cone, ref)
            assert nf.nonfinite(ref)[cone].all() and np.array_equal(ref[~cone], clean[~cone])
            if rule == "torch":
                got = lr.max_pool(xp, 3, stride, 1)
                assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~cone], ref[~cone])


def test_pool_grad_reference_carries_dy():
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (1, 9, 9, 64)).astype(np.float32)
    dy = rng.normal(0, 1, (1, 5, 5, 64)).astype(np.float32)
    for avg in (False, True):
        clean = nf.pool_grad_ref(x, dy, 3, 2, avg)
        d = dy.copy()
        d[0, 2, 2, 9] = NAN
        ref = nf.pool_grad_ref(x, d, 3, 2, avg)
        cone = nf.pool_grad_cone(x, 3, 2, avg, (2, 2, 9))
        nf.check_placement(cone, ref)
        assert np.isnan(ref[cone]).all() and np.array_equal(ref[~cone], clean[~cone])


def test_layer_oracles_carry_nan():
    rng = np.random.default_rng(1)
    feat = rng.normal(0, 1, (2, 25, 64)).astype(np.float32)
    feat[0, 7, 5] = NAN
    w = rng.normal(0, 0.2, (5, 64)).astype(np.float32)
    for use_max in (False, True):
        score, pooled = lr.gap_linear_sigmoid(feat, w, None, use_max, 1)
        assert np.isnan(pooled[0, 5]) and np.isfinite(np.delete(pooled, 5, axis=1)).all()
        assert np.isnan(score[0]).all() and np.isfinite(score[1]).all()
    head = rng.normal(0, 1, (2, 5, 5, 8)).astype(np.float32)
    head[1, 2, 4, 3] = NAN
    cam = lr.flip_add(head, 8)
    assert np.isnan(cam[0, 3, 2, 0]) and np.isnan(cam).sum() == 1  # (the flipped half: column w - 1 - 4)
    x = rng.normal(0, 1, (2, 5, 5, 64)).astype(np.float32)
    x[1, 0, 0, 40] = NAN
    y = lr.group_norm_head(x, np.ones(64), np.zeros(64), 4, 1e-5, 1, True, 5, 5, np.zeros((2, 5, 5, 64)), 0)
    assert np.isnan(y[1, :, :, 32:48]).all() and np.isnan(y).sum() == 25 * 16  # its (sample, group) and nothing else
    z = rng.normal(0, 1, (50, 5))
    z[3, 2] = NAN
    z[4, 1] = PINF
    z[5, 0] = NINF
    p = nf.fc8_softmax_ref(z, 1e-4)
    assert np.isnan(p[3]).all() and np.isnan(p[4]).all() and np.isfinite(np.delete(p, (3, 4), axis=0)).all()  # exp(-inf) = 0: finite


@pytest.mark.parametrize("kind", ["mean", "max"])
def test_cls_head_oracle_carries_nan(kind):
    """A NaN score is NaN through K.clip, the log and the clip's gradient mask times the sigmoid's NaN derivative: the loss and the
    poisoned sample's gradients are NaN, the other sample's feature gradient is finite."""
    feat, w, bias, target, _ = cls_head_ref.make_case((2, 9, 64, 5), kind, with_weights=False)
    f = feat.copy()
    f[0, 4, 10] = NAN
    r = cls_head_ref.cls_loss(f, kind, w, bias, target)
    assert np.isnan(r["values"]["loss"]) and np.isnan(r["values"]["mean_loss"])
    assert np.isnan(r["p"][0]).all() and np.isfinite(r["p"][1]).all()
    assert np.isnan(r["g_bias"]).all() and np.isnan(r["g_w"]).all()
    assert np.isfinite(r["g_feat"][1]).all()
    assert np.isnan(r["g_feat"][0]).all() if kind == "mean" else np.isnan(r["g_feat"][0]).any()
    wn = w.copy()
    wn[2, 7] = NAN
    r = cls_head_ref.cls_loss(feat, kind, wn, bias, target)
    assert np.isnan(r["values"]["loss"]) and np.isnan(r["p"][:, 2]).all() and np.isfinite(np.delete(r["p"], 2, axis=1)).all()
    assert np.isnan(r["g_bias"][2]) and np.isfinite(np.delete(r["g_bias"], 2)).all()
    assert np.isnan(r["g_w"][2]).all() and np.isfinite(np.delete(r["g_w"], 2, axis=0)).all()


def test_sgd_oracles_poison_one_element():
    rng = np.random.default_rng(2)
    n = 40
    p, g, acc, mom = (rng.normal(0, 1, n).astype(np.float32) for _ in range(4))
    segs = [("a.w", 0, 30, 1.0, True), ("a.b", 30, 40, 2.0, False)]
    for value in nf.POISONS.values():
        for at in (3, 35):
            gp = g.copy()
            gp[at] = value
            a0 = seg_sgd_ref.accumulate(segs, p, g, acc, 5e-4, 1)
            a1 = seg_sgd_ref.accumulate(segs, p, gp, acc, 5e-4, 1)
            p0, _, m0 = seg_sgd_ref.apply(p, a0, mom, 1e-4, 0.9)
            p1, _, m1 = seg_sgd_ref.apply(p, a1, mom, 1e-4, 0.9)
            for clean, got in ((a0, a1), (p0, p1), (m0, m1)):
                assert not np.isfinite(got[at]) and np.array_equal(np.delete(got, at).view(np.uint32), np.delete(clean, at).view(np.uint32))
            q0, n0 = irn_sgd_ref.sgd_step32(p, g, mom, 30, 0.1, 1.0, 1e-4, 0.9)
            q1, n1 = irn_sgd_ref.sgd_step32(p, gp, mom, 30, 0.1, 1.0, 1e-4, 0.9)
            for clean, got in ((q0, q1), (n0, n1)):
                assert not np.isfinite(got[at]) and np.array_equal(np.delete(got, at).view(np.uint32), np.delete(clean, at).view(np.uint32))


def test_loss_oracles_carry_nan():
    """tests/seg_loss_ref.py and tests/irn_loss_ref.py: one NaN probability / edge logit / displacement is a NaN total"""
    from tests import irn_loss_ref, seg_loss_ref

    prob, crf, cues, labels = seg_loss_ref.make_case((3, 7, 5, 5))
    p = prob.copy()
    p[0, 3, 2, 1] = NAN
    for method in ("SEC", "DSRG"):
        assert np.isnan(seg_loss_ref.evaluate(method, p, crf, cues, labels)[0]["norm"])
    case = irn_loss_ref.CASES[1]
    edge, dp, label = irn_loss_ref.make_case(case)
    e, d = edge.copy(), dp.copy()
    e[0, 4, 5] = NAN
    d[1, 0, 4, 5] = NAN
    assert np.isnan(irn_loss_ref.tensor_form(e, dp, label, case[0], grad=False)["loss"]["total"])
    assert np.isnan(irn_loss_ref.tensor_form(edge, d, label, case[0], grad=False)["loss"]["total"])


def test_relu_bias_grad_reference():
    rng = np.random.default_rng(3)
    y, dy = rng.normal(0, 1, (81, 64)), rng.normal(0, 1, (81, 64)).astype(np.float32)
    dy[40, 3] = NAN
    y[40, 3] = 1.0
    dz, db = nf.relu_bias_grad_ref(y, dy)
    assert np.isnan(dz[40, 3]) and np.isnan(dz).sum() == 1 and np.isnan(db[3]) and np.isfinite(np.delete(db, 3)).all()


# (first words of the row's first cell in DESIGN.md 5.1, the entry as nonfinite_ref.outcome names it, its operand / Cin)
TABLE_ROWS = [("`wsc_net_create`", "net_create", None, 64), ("every whole-net forward", "net", None, 64),
              ("`wsc_net_seg_load_params`", "load_params", None, 64), ("`SegTrainer.step`", "trainer_step", None, 64),
              ("`wsc_conv2d_nchw(_dil)`: input", "conv2d_nchw", "x", 64), ("`wsc_conv2d_nchw(_dil)`: weight", "conv2d_nchw", "w", 64),
              ("`wsc_maxpool_nhwc`", "pool", None, 64), ("`wsc_maxpool_nhwc`", "gap_linear_sigmoid", None, 64),
              ("`wsc_group_norm_nhwc`", "group_norm_nhwc", None, 64), ("`wsc_cam_flip_add`", "cam_flip_add", None, 64),
              ("`wsc_cam_flip_add`", "fc8_softmax", None, 64), ("`wsc_cam_flip_add`", "pool_same_grad", None, 64),
              ("`wsc_cam_flip_add`", "relu_bias_grad", None, 64), ("`wsc_cam_flip_add`", "conv2d_wgrad", None, 64),
              ("`wsc_cam_flip_add`", "conv2d_dgrad", None, 64), ("`wsc_cls_loss`", "cls_loss", None, 64),
              ("`wsc_seg_loss`", "seg_loss", None, 64), ("`wsc_seg_loss`", "irn_aff_loss", None, 64),
              ("`wsc_seg_sgd_accumulate`", "seg_sgd", None, 64), ("`wsc_seg_sgd_accumulate`", "irn_sgd", None, 64)]


def test_outcome_table():
    """nonfinite_ref.outcome -- what the GPU tests assert -- is the table of DESIGN.md section 5.1, row by row"""
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    rows = [[c.strip() for c in line.strip().strip("|").split("|")] for line in text.splitlines() if line.startswith("| ")]
    rows = [r for r in rows if len(r) == 3]
    for first, entry, operand, cin in TABLE_ROWS:
        hit = [r for r in rows if r[0].startswith(first)]
        assert len(hit) == 1, first
        for col, prec in ((1, _lib.PREC_F16), (1, _lib.PREC_F16X3), (2, _lib.PREC_BF16), (2, _lib.PREC_BF16X3), (2, _lib.PREC_F32)):
            assert hit[0][col].startswith(nf.outcome(entry, prec, operand, cin)), (first, entry, lr.PREC_NAME[prec], hit[0][col])
    small = [r for r in rows if r[0].startswith("`wsc_conv2d_nchw(_dil)`: input")][0][2]
    assert "Cin <= 4" in small and "bf16 / bf16x3: L" in small
    for prec in lr.ALL_PRECISIONS:
        assert nf.outcome("conv2d_nchw", prec, "x", 3) == ("P" if prec == _lib.PREC_F32 else "L")
        assert nf.outcome("conv2d_nchw", prec, "w", 3) == nf.outcome("conv2d_nchw", prec, "w", 64)
    with pytest.raises(KeyError):
        nf.outcome("no such entry", _lib.PREC_F32)
