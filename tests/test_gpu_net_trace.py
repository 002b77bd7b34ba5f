"""GPU: every op of a forward pass on its own inputs.  wsc_net_forward_trace runs the production launch sequence of a net and hands
out each op's output as float32 (hi + lo of the two-plane modes: exact); the float64 closure of the op's label (tests/
net_trace_ref.py) is fed the DEVICE's traced outputs of the op's producers -- exactly what the op read -- and every element of
what the op wrote is compared.  So an error of one op is seen at that op, at the size of one op's rounding, instead of after 53
layers at the end-to-end bounds of tests/test_gpu_net.py.

Pools and gathers: equality.  Convs and the head: net_trace_ref.asserted_bound = min(the bound derived from the arithmetic --
its docstring states every term --, the bound tests/test_gpu_conv.py holds the same launcher to at that precision); the exact
fp32 mode has the derived bound alone.  Each case prints its worst err / bound per op kind.  Structure: the plan's labels and
producers are the host's list, the last entry of the stack is wsc_net_forward_features, a traced run leaves the CAM's bits alone,
the fused stem + max-pool equals the unfused pair entry for entry, and both CAM heads meet the head's bound."""
import functools

import numpy as np
import pytest
import torch

from oracle import cnn_ref
from tests import deeplab_ref, layer_ref
from tests import net_trace_ref as nt
from wsscam import _lib, secdsrg

pytestmark = pytest.mark.gpu

PREC = {"f16x3": _lib.PREC_F16X3, "f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "f16": _lib.PREC_F16}
U = 2.0 ** -24
C = 20


def _trace(ctx, net, x, N, H, W, skip=()):
    """-> (plan, entries): entries[i] the float32 [N][Ho][Wo][pitch] tensor op i wrote into, None where the run has none"""
    plan = net.trace_plan(N, H, W, ctx)
    off, total = [], 0
    for i, p in enumerate(plan):
        if p["fused_next"] or i in skip:
            off.append(-1)
            continue
        off.append(total)
        total += N * p["Ho"] * p["Wo"] * p["pitch"]
    x_dev, t_dev = ctx.to_device(np.ascontiguousarray(x)), ctx.alloc(total * 4)
    try:
        net.forward_trace(x_dev, N, H, W, off, t_dev, total, ctx)
        flat = ctx.to_host(t_dev, (total,), np.float32)
    finally:
        x_dev.free()
        t_dev.free()
    assert ctx.range_status() == 0
    ent = [None if o < 0 else flat[o:o + N * p["Ho"] * p["Wo"] * p["pitch"]].reshape(N, p["Ho"], p["Wo"], p["pitch"]) for o, p in zip(off, plan)]
    return plan, ent


def _t(nhwc):
    return torch.from_numpy(np.ascontiguousarray(nhwc)).double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _check_structure(plan, layers):
    assert [p["label"] for p in plan] == [ly.label for ly in layers]  # no layer skipped, none twice
    kinds = {"conv": _lib.TRACE_CONV, "pool": _lib.TRACE_POOL, "gather": _lib.TRACE_GATHER, "head": _lib.TRACE_HEAD}
    for i, (p, ly) in enumerate(zip(plan, layers)):
        assert p["kind"] == kinds[ly.kind], (i, p)
        for key in ("in", "in2", "res"):
            assert p[key] < i and p[key] >= _lib.TRACE_NONE, (i, key, p)  # an earlier op, the input, or none
        assert (p["in"], p["in2"], p["res"]) == tuple(ly.inputs), (i, p["label"], p, ly.inputs)
        if ly.kind == "pool":
            assert (p["pool_rule"], p["pool_k"], p["pool_stride"], p["pool_pad"], p["pool_avg"]) == ly.pool, (p, ly.pool)
        assert p["affine2"] == (ly.steps == 4) and (p["stride2"] > 0) == (p["in2"] != _lib.TRACE_NONE)
        assert 0 <= p["coff"] and p["coff"] + p["C"] <= p["pitch"]


def _check_ops(plan, ent, layers, x_nchw, prec, what):
    """every op of a traced run against its closure on the device's own operands -> {kind: worst err / bound}"""
    x_in = _t(layer_ref.as_precision(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1)), PREC[prec]))  # what the input planes hold
    worst, binding = {}, [0, 0]

    def operand(j):
        return x_in if j == nt.INPUT else (None if j == nt.NONE else _t(ent[j]))

    def conv_like(ly, p, a, b, c):
        ref, A, S = [t.numpy() for t in ly.fn(a, b, c)]
        bound, derived, table = nt.asserted_bound(prec, ly, ref, A, S, f32_out=ly.kind == "head")
        return ref, bound, derived, table

    for i, (p, ly) in enumerate(zip(plan, layers)):
        if p["fused_next"]:
            continue
        got = ent[i][..., p["coff"]:p["coff"] + p["C"]].astype(np.float64)
        fused_stem = p["in"] >= 0 and plan[p["in"]]["fused_next"]
        if ly.kind == "gather":
            ref = _nhwc(ly.fn(operand(p["in"]))[0])
            assert got.shape == ref.shape and np.array_equal(got, ref), (what, p["label"])
            first = plan[ly.concat_with]  # ... beside the channels the conv before it wrote, untouched
            assert np.array_equal(ent[i][..., :first["C"]], ent[ly.concat_with][..., :first["C"]]), (what, p["label"])
            continue
        if ly.kind == "pool" and not fused_stem:
            ref = _nhwc(ly.fn(operand(p["in"]))[0])
            assert got.shape == ref.shape, (what, p["label"], got.shape, ref.shape)
            if p["pool_avg"]:
                # the kernel sums and divides in double and rounds once to fp32 (2^-24 |ref|); the two-plane modes then split
                # the result (relative 2^-22 in f16x3, 2^-16 in bf16x3; + half a half-subnormal spacing, 2^-25, in f16x3)
                split = {"f32": 0.0, "f16x3": 2.0 ** -22, "bf16x3": 2.0 ** -16, "f16": 2.0 ** -11}[prec]
                bound = (U + split) * np.abs(ref) + (2.0 ** -25 if prec in ("f16x3", "f16") else 0.0)
                r = (np.abs(got - ref) / bound).max()
                worst["avgpool"] = max(worst.get("avgpool", 0.0), r)
                assert r <= 1.0, (what, p["label"], r)
            else:
                assert np.array_equal(got, ref), (what, p["label"], np.abs(got - ref).max())
            continue
        if fused_stem:
            # conv + BN + ReLU + max-pool in one kernel: a maximum moves by at most the largest error of its window
            stem = layers[p["in"]]
            q = plan[p["in"]]
            ref_c, bound_c, derived, table = conv_like(stem, q, operand(q["in"]), None, None)
            ref = _nhwc(ly.fn(torch.from_numpy(ref_c))[0])
            bound = _nhwc(ly.fn(torch.from_numpy(bound_c))[0])
            kind = "stem+pool"
        else:
            ref, bound, derived, table = conv_like(ly, p, operand(p["in"]), operand(p["in2"]), operand(p["res"]))
            ref, bound = ref.transpose(0, 2, 3, 1), bound.transpose(0, 2, 3, 1)
            kind = "head" if ly.kind == "head" else ("entry" if ly.entry else ("conv+affine2" if p["affine2"] else "conv"))
        assert got.shape == ref.shape, (what, p["label"], got.shape, ref.shape)
        if table is not None:
            binding[0] += int((derived <= table).sum())
            binding[1] += derived.size
        err = np.abs(got - ref)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst[kind] = max(worst.get(kind, 0.0), float(ratio.max()))
        bad = err > bound
        assert not bad.any(), "%s op %d %s: %d of %d beyond the bound, worst err / bound %.3g at %s (|ref| there %.3g, max|ref| %.3g)" % (
            what, i, p["label"], bad.sum(), bad.size, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape), np.abs(ref).flat[ratio.argmax()],
            np.abs(ref).max())
    print("net trace %s: worst err / bound %s; derived bound is the smaller one on %.1f%% of the elements" % (
        what, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), 100.0 * binding[0] / max(binding[1], 1)))
    return worst


def _net(ctx, arch, sd, prec):
    return _lib.Net(ctx, arch, {k: np.asarray(v, dtype=np.float32) for k, v in sd.items()}, C, PREC[prec])


# ---- ResNet50 CAM ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _resnet_sd(extreme):
    return nt.extreme_bn_state_dict(C) if extreme else cnn_ref.make_resnet50_cam_state_dict(C, seed=0)


def _resnet_x(N, hw):
    return np.random.default_rng(hw[0] * 100 + hw[1]).normal(0, 1, (N, 3) + hw).astype(np.float32)


RESNET_CASES = [(prec, hw, False) for prec in ("f16x3", "f32", "bf16x3", "f16") for hw in ((65, 97), (64, 64))] + [("f16x3", (65, 97), True)]


@pytest.mark.parametrize("prec, hw, extreme", RESNET_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_resnet50_every_op(ctx, prec, hw, extreme):
    """N = 3 (ragged row tiles); 65 x 97 strides odd maps in layers 2 and 3 (17 x 25 -> 9 x 13 -> 5 x 7): the second source of the
    stage entry on sizes where an off-by-one shows.  f16x3 / f16: the two-source stage entry; f32: separate projection + residual;
    bf16x3: conv2 into a channel range + gather; f16: the one-plane head.  extreme: BatchNorm scales that are zero, negative and
    five orders of magnitude apart on every stage entry -- A carries the scale, so the bound means something per element."""
    sd = _resnet_sd(extreme)
    layers = nt.resnet50_layers(sd, prec)
    net = _net(ctx, _lib.ARCH_RESNET50_CAM, sd, prec)
    try:
        x = _resnet_x(3, hw)
        plan, ent = _trace(ctx, net, x, 3, hw[0], hw[1])
        _check_structure(plan, layers)
        if hw == (65, 97):
            sizes = [(p["Ho"], p["Wo"]) for p in plan if p["label"].endswith(".0.conv3+downsample") or p["label"].endswith(".0.conv3")]
            assert sizes == [(17, 25), (9, 13), (5, 7), (5, 7)]
        assert plan[0]["fused_next"] == (prec in ("f16x3",)) and sum(p["fused_next"] for p in plan) == plan[0]["fused_next"]
        worst = _check_ops(plan, ent, layers, x, prec, "resnet50 %s %dx%d%s" % (prec, hw[0], hw[1], " extreme-bn" if extreme else ""))
        assert set(worst) >= {"conv", "head"} and ("entry" in worst) == (prec != "f32")
        if hw[0] == hw[1]:  # the last entry of the stack is the feature map the library returns
            x_dev, f_dev = ctx.to_device(x), ctx.alloc(ent[-2].nbytes)
            net.forward_features(x_dev, 3, hw[0], f_dev)
            assert np.array_equal(ctx.to_host(f_dev, ent[-2].shape, np.float32).view(np.uint32), ent[-2].view(np.uint32))
            x_dev.free()
            f_dev.free()
    finally:
        net.close()


def test_resnet50_traced_run_leaves_the_cam_alone_and_head_is_the_cam(ctx):
    """wsc_net_forward_cam_hw before and after a traced run: the same bits; and the CAM is the [orig, flip] pair sum of the ReLU
    of the traced head (resnet50_cam.py:65-66) -- one fp32 add, so again the same bits."""
    sd = _resnet_sd(False)
    net = _net(ctx, _lib.ARCH_RESNET50_CAM, sd, "f16x3")
    try:
        B, (H, W) = 3, (65, 97)
        x = np.random.default_rng(5).normal(0, 1, (B, 2, 3, H, W)).astype(np.float32)
        hh, ww = net.cam_size_hw(H, W)
        x_dev, c_dev = ctx.to_device(x), ctx.alloc(B * C * hh * ww * 4)

        def cam():
            net.forward_cam_hw(x_dev, B, H, W, c_dev)
            return ctx.to_host(c_dev, (B, C, hh, ww), np.float32)

        before = cam()
        n_ops = len(net.trace_plan(2 * B, H, W, ctx))
        plan, ent = _trace(ctx, net, x.reshape(2 * B, 3, H, W), 2 * B, H, W, skip=range(n_ops - 2))
        after = cam()
        x_dev.free()
        c_dev.free()
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        assert np.array_equal(layer_ref.flip_add(ent[-1], C), before) and before.max() > 0
        # ... and the head's own bound on the ragged M = 6 * 35 rows
        layers = nt.resnet50_layers(sd, "f16x3")
        ref, A, S = [t.numpy().transpose(0, 2, 3, 1) for t in layers[-1].fn(_t(ent[-2]))]
        bound, _, _ = nt.asserted_bound("f16x3", layers[-1], ref, A, S, f32_out=True)
        assert (np.abs(ent[-1] - ref) <= bound).all(), (np.abs(ent[-1] - ref) / bound).max()
    finally:
        net.close()


def test_resnet50_fused_stem_entries_equal_unfused_and_both_heads_in_bound(ctx):
    sd = _resnet_sd(False)
    layers = nt.resnet50_layers(sd, "f16x3")
    net = _net(ctx, _lib.ARCH_RESNET50_CAM, sd, "f16x3")
    try:
        hw = (65, 97)
        x = _resnet_x(3, hw)
        plan_f, ent_f = _trace(ctx, net, x, 3, hw[0], hw[1], skip=range(2, len(layers) - 2))
        with ctx.option(_lib.OPT_STEM_POOL_FUSED, 0):
            plan_u, ent_u = _trace(ctx, net, x, 3, hw[0], hw[1], skip=range(2, len(layers) - 2))
        assert plan_f[0]["fused_next"] == 1 and ent_f[0] is None
        assert plan_u[0]["fused_next"] == 0 and ent_u[0] is not None  # the stem conv as an entry of its own
        assert [dict(p, fused_next=0) for p in plan_f] == plan_u
        for i in (1, len(layers) - 2, len(layers) - 1):  # the pool, the feature map, the head
            assert np.array_equal(ent_f[i].view(np.uint32), ent_u[i].view(np.uint32)), plan_f[i]["label"]
        # the unfused stem and its pool on their own
        _check_ops(plan_u[:2], ent_u[:2], layers[:2], x, "f16x3", "resnet50 f16x3 unfused stem")
        # the streaming head (K summed in four per-wave quarters) and the tiled head: two summation orders, one bound
        with ctx.option(_lib.OPT_CAM_HEAD_STREAM, 0):
            _, ent_t = _trace(ctx, net, x, 3, hw[0], hw[1], skip=range(len(layers) - 2))
        assert np.array_equal(ent_t[-2].view(np.uint32), ent_f[-2].view(np.uint32))
        ref, A, S = [t.numpy().transpose(0, 2, 3, 1) for t in layers[-1].fn(_t(ent_f[-2]))]
        bound, _, _ = nt.asserted_bound("f16x3", layers[-1], ref, A, S, f32_out=True)
        for name, e in (("stream", ent_f[-1]), ("tiled", ent_t[-1])):
            r = (np.abs(e - ref) / bound).max()
            print("resnet50 f16x3 head (%s): worst err / bound %.3f" % (name, r))
            assert r <= 1.0, (name, r)
    finally:
        net.close()


# ---- the plain stacks ----------------------------------------------------------------------------------------------------------------
def _plain_case(kind):
    """-> (arch, state dict for the library, layers builder)"""
    if kind in ("vgg16-bn", "vgg16"):
        sd = nt.odd_s2_state_dict(C) if kind == "vgg16-bn" else cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, C, False, seed=6)
        build = lambda prec: nt.plain_layers(sd, "vgg16", cnn_ref.VGG16_CFG, head_w=sd["vgg16.classifier.0.weight"][:C], prec=prec)
        return _lib.ARCH_VGG16_CAM, dict(sd), build
    sd = cnn_ref.make_plain_state_dict("m7", cnn_ref.M7_CFG, C, True, seed=7)
    alpha = torch.randn(256, C, generator=torch.Generator().manual_seed(8)) * 0.05  # Grad-CAM weights (F, C)
    lib_sd = dict(sd, gradcam_weights=alpha)
    pools = None
    if kind == "m7-pool_spec":
        pools = [(3, 2, 1), (2, 2, 0), (2, 2, 0)]  # 3 / 2 SAME, 2 / 2 VALID; the third row is the classifier branch's
        lib_sd["pool_spec"] = np.asarray(pools, np.float32)
    build = lambda prec: nt.plain_layers(sd, "m7", cnn_ref.M7_CFG, pools=pools, head_w=alpha.t(), prec=prec)
    return _lib.ARCH_M7_CAM, lib_sd, build


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("kind", ["vgg16-bn", "vgg16", "m7", "m7-pool_spec"])
def test_plain_stack_every_op(ctx, kind, prec):
    """conv -> bias -> ReLU -> BatchNorm(eps 1e-3) of every VGG16-BN / M7 layer (ConvW::s2 / b2: the second affine map, after the
    ReLU) -- vgg16-bn with negative and tiny scales on some channels of every layer --, the in-network pools (a pool_spec net: TF
    SAME 3 / 2 and VALID 2 / 2), the small-Cin first layer and the 1x1 head, at 33 x 37."""
    arch, lib_sd, build = _plain_case(kind)
    layers = build(prec)
    net = _net(ctx, arch, lib_sd, prec)
    try:
        H, W = 33, 37
        x = np.random.default_rng(len(kind)).normal(0, 1, (3, 3, H, W)).astype(np.float32)
        plan, ent = _trace(ctx, net, x, 3, H, W)
        _check_structure(plan, layers)
        worst = _check_ops(plan, ent, layers, x, prec, "%s %s 33x37" % (kind, prec))
        assert ("conv+affine2" in worst) == (kind != "vgg16") and "head" in worst
        if kind == "m7-pool_spec":
            assert [(p["pool_rule"], p["pool_k"], p["pool_stride"]) for p in plan if p["kind"] == _lib.TRACE_POOL] == [(1, 3, 2), (2, 2, 2)]
            assert (plan[-1]["Ho"], plan[-1]["Wo"]) == (8, 9)  # 33 -> 17 -> 8, 37 -> 19 -> 9
    finally:
        net.close()


# ---- DeepLab-LFOV trunk ------------------------------------------------------------------------------------------------------------
def test_deeplab_trunk_every_op(ctx):
    """a thin DeepLab-LFOV (every width 64) at 41 x 41 in f16x3: the NHWC input, the rate-2 convs, the TF-SAME max pools at stride
    2 and 1 (equality), and the 3 x 3 average pool at its own bound.  The fc6 - fc8 branch runs behind the stack and is not traced."""
    wts = deeplab_ref.random_weights("SEC", 5, 64, 128, seed=7)
    x = deeplab_ref.net_input(3, 41, 41, 8)
    layers = nt.deeplab_layers(wts)
    net = _lib.Net(ctx, _lib.ARCH_DEEPLAB_LFOV, secdsrg.seg_state_dict("SEC", wts, 5), 5, _lib.PREC_F16X3)
    try:
        plan, ent = _trace(ctx, net, x, 3, 41, 41)
        _check_structure(plan, layers)
        assert [p["dil"] for p in plan if p["kind"] == _lib.TRACE_CONV] == [1] * 10 + [2] * 3
        worst = _check_ops(plan, ent, layers, np.ascontiguousarray(x.transpose(0, 3, 1, 2)), "f16x3", "deeplab-lfov f16x3 41x41")
        assert "avgpool" in worst and "conv" in worst
        assert ent[-1].shape == (3,) + net.seg_size_hw(41, 41) + (64,)
    finally:
        net.close()


def test_trace_entry_rejects_what_it_cannot_serve(ctx):
    sd = _resnet_sd(False)
    net = _net(ctx, _lib.ARCH_RESNET50_CAM, sd, "f16x3")
    try:
        plan = net.trace_plan(1, 64, 64, ctx)
        skip = [-1] * len(plan)
        x_dev, t_dev = ctx.to_device(np.zeros((1, 3, 64, 64), np.float32)), ctx.alloc(4096)
        for off in (skip[:-1], [0] + skip[1:], skip[:-1] + [1024 - 1 * 4 * 4 * C + 1]):  # a short list, the fused stem, past the buffer's end
            with pytest.raises(_lib.WscError) as ei:
                net.forward_trace(x_dev, 1, 64, 64, off, t_dev, 1024, ctx)
            assert ei.value.status == _lib.WSC_ERR_INVALID
        net.forward_trace(x_dev, 1, 64, 64, skip[:-1] + [1024 - 1 * 4 * 4 * C], t_dev, 1024, ctx)  # ... and the last place that fits
        ctx.sync()
        x_dev.free()
        t_dev.free()
    finally:
        net.close()
