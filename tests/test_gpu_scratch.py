"""GPU: no result may depend on what scratch memory held before the call ("Scratch memory").

Every public entry point that takes scratch -- the grow-only workspace arena, a cached block, a staged table -- runs four times on
the same inputs: with the context's scratch fill off, and with the arena (at every request of an entry point), every cached block
handed out and the gradient objects' own workspaces set to 0x00, to 0xFF
(NaN as fp32 / fp16 / bf16, -1 as int32, the maximum as a counter) and to 0x3F (0.747 as fp32, 1.81 as fp16: finite, so it shows in
a sum and is not swallowed by fmaxf, a ReLU or a comparison the way NaN is).  Every buffer the caller hands in is allocated with a
guard band on either side and pre-filled, bands included, with the run's byte (0xA5 for the run without a fill).  Asserted:
  * the guard bands come back untouched;
  * the four runs agree bit for bit -- which also says that every output cell was written: a cell the call left alone holds four
    different bytes in the four runs.
There is no tolerance in this file: the comparisons against the oracles stay where they are.

CASES maps every entry point to the cases that reach it; tests/test_scratch_table_host.py holds the table against the header.
"""
import contextlib
import functools

import numpy as np
import pytest

from wsscam import _lib

pytestmark = pytest.mark.gpu

OFF = -1
FILLS = (OFF, 0x00, 0xFF, 0x3F)
PREFILL = {OFF: 0xA5, 0x00: 0x00, 0xFF: 0xFF, 0x3F: 0x3F}
GUARD = 256  # bytes on either side of every caller buffer (a multiple of 256: the buffers keep hipMalloc's alignment)

# entry point -> [case id]; case id -> (function, fresh context?)
CASES = {}
_RUNS = {}


def case(cid, *entries, fresh=False):
    """Registers `fn(ctx) -> [host arrays]` under the entry points it reaches.  fresh: every run gets a context of its own (the
    per-context caches -- the Gaussian lattices -- are then built under the fill as well)."""
    def deco(fn):
        assert cid not in _RUNS, cid
        _RUNS[cid] = (fn, fresh)
        for e in entries:
            assert e.startswith("wsc_"), e
            CASES.setdefault(e, []).append(cid)
        return fn
    return deco


class _GuardedBuffer(_lib.DeviceBuffer):
    """A caller buffer between two guard bands, all of it set to `byte`; the bands are read back when it is freed."""

    def __init__(self, ctx, nbytes, byte, log):
        super().__init__(ctx, int(nbytes) + 2 * GUARD)
        self._base, self._byte, self._log = self.ptr, byte, log
        self.ptr, self.nbytes = self._base + GUARD, int(nbytes)
        _lib.check(ctx._lib.wsc_memset(ctx.h, self._base, byte, self.nbytes + 2 * GUARD))

    def check_bands(self):
        for what, at in (("before", self._base), ("behind", self._base + GUARD + self.nbytes)):
            band = self.ctx.to_host(at, (GUARD,), np.uint8)
            if not (band == self._byte).all():
                self._log.append("a store %s a caller buffer of %d bytes (%d guard bytes changed)" % (what, self.nbytes, int((band != self._byte).sum())))

    def free(self):
        if getattr(self, "_base", None) and self.ctx.h:
            self.check_bands()
            self.ctx._lib.wsc_free(self.ctx.h, self._base)
        self._base = self.ptr = None


@contextlib.contextmanager
def guarded_allocations(ctx, byte):
    """Inside the block every ctx.alloc / ctx.to_device buffer is a _GuardedBuffer; leaving it checks the bands of the ones still
    alive and raises on any band a call wrote to."""
    log, live = [], []

    def alloc(nbytes, pooled=False):
        live.append(_GuardedBuffer(ctx, nbytes, byte, log))
        return live[-1]

    ctx.alloc = alloc
    try:
        yield
        for buf in live:
            buf.free()
        assert not log, log
    finally:
        del ctx.alloc  # (the class's method again)
        for buf in live:
            buf._log = []
            buf.free()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def run_once(ctx, fn, fill):
    with guarded_allocations(ctx, PREFILL[fill]):
        if fill == OFF:
            out = fn(ctx)
        else:
            with ctx.scratch_fill(fill):
                out = fn(ctx)
                ctx.sync()
        return [np.array(o, copy=True) for o in out]


def sweep(shared_ctx, cid):
    fn, fresh = _RUNS[cid]
    outs = {}
    for fill in FILLS:
        ctx = _lib.Context(0) if fresh else shared_ctx
        try:
            outs[fill] = run_once(ctx, fn, fill)
        finally:
            if fresh:
                ctx.close()
    base = outs[OFF]
    assert len(base) > 0 and all(o.size > 0 for o in base), cid
    for fill in FILLS[1:]:
        assert len(outs[fill]) == len(base)
        for k, (a, b) in enumerate(zip(base, outs[fill])):
            assert a.shape == b.shape and a.dtype == b.dtype, (cid, k)
            diff = bits(a) != bits(b)
            assert not diff.any(), "%s: output %d differs under scratch fill 0x%02X in %d of %d words, first at %s: 0x%x vs 0x%x" % (
                cid, k, fill, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist(), int(bits(a)[diff][0]), int(bits(b)[diff][0]))


def out(ctx, shape, dtype=np.float32):
    return ctx.alloc(int(np.prod(shape)) * np.dtype(dtype).itemsize)


def host(ctx, buf, shape, dtype=np.float32):
    return ctx.to_host(buf, shape, dtype)


# ---- single conv layers ------------------------------------------------------------------------------------------------------------
PRECS = {"bf16": _lib.PREC_BF16, "bf16x3": _lib.PREC_BF16X3, "f16": _lib.PREC_F16, "f16x3": _lib.PREC_F16X3, "f32": _lib.PREC_F32}
# rows of test_gpu_conv.SHAPES: the stem, the VGG first layer, a partial column tile with ragged M, the workspace-carving row, one
# K-step strided; an LDS-window shape of test_conv_lds_window_equals_per_tap_staging at k = 3; (N, Cin, H, W, Cout, k, stride, pad)
CONV_SHAPES = [(2, 3, 65, 65, 64, 7, 2, 3), (2, 3, 33, 37, 64, 3, 1, 1), (5, 128, 7, 9, 136, 1, 1, 0), (2, 64, 9, 11, 72, 3, 1, 1),
               (2, 64, 16, 16, 64, 1, 2, 0), (5, 64, 7, 9, 128, 3, 1, 1)]
DIL_ROW = (13, 11, 6)  # test_gpu_deeplab.DIL_SHAPES[1]


@functools.lru_cache(maxsize=None)
def _conv_data(shape, dil=1):
    N, Cin, H, W, Cout, k, stride, pad = shape
    rng = np.random.default_rng(sum(shape) + dil)
    x = rng.normal(0, 1, (N, Cin, H, W)).astype(np.float32)
    w = (rng.normal(0, 1, (Cout, Cin, k, k)) * np.sqrt(2.0 / (Cin * k * k))).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    Ho, Wo = (H + 2 * pad - ((k - 1) * dil + 1)) // stride + 1, (W + 2 * pad - ((k - 1) * dil + 1)) // stride + 1
    res = rng.normal(0, 1, (N, Cout, Ho, Wo)).astype(np.float32)
    return x, w, scale, shift, res


def _conv_case(shape, prec, dil=1):
    def fn(ctx):
        N, Cin, H, W = shape[:4]
        x, w, scale, shift, res = _conv_data(shape, dil)
        outs = []
        x_dev, r_dev = ctx.to_device(x), ctx.to_device(res)
        for use_res, relu in ((False, False), (True, True)):
            y_dev, shp = _lib.conv2d_nchw(ctx, x_dev, N, Cin, H, W, w, shape[6], shape[7], scale, shift, r_dev if use_res else None, relu,
                                          prec, dil=dil)
            outs.append(host(ctx, y_dev, shp))
        return outs
    return fn


for _name, _p in PRECS.items():
    for _s in CONV_SHAPES:
        case("conv-%s-%s" % ("x".join(map(str, _s)), _name), "wsc_conv2d_nchw")(_conv_case(_s, _p))
    _s = (2, 64, DIL_ROW[0], DIL_ROW[1], 64, 3, 1, DIL_ROW[2])
    case("conv-dil%d-%s" % (DIL_ROW[2], _name), "wsc_conv2d_nchw_dil")(_conv_case(_s, _p, dil=DIL_ROW[2]))


# ---- single layers -----------------------------------------------------------------------------------------------------------------
def _pool_input(C=72):
    return (np.random.default_rng(7).normal(0, 3, (3, 7, 9, C)) - 1.0).astype(np.float32)


def _pool_case(entry_name, arg_sets):
    def fn(ctx):
        entry = getattr(_lib, entry_name)
        outs = []
        for C in (8, 72):
            x = _pool_input(C)
            x_dev = ctx.to_device(x)
            N, H, W, _ = x.shape
            for prec in PRECS.values():
                for args in arg_sets:
                    y_dev, shp = entry(ctx, x_dev, N, H, W, C, *args, prec)
                    outs.append(host(ctx, y_dev, shp))
                    y_dev.free()
        return outs
    return fn


case("maxpool-nhwc", "wsc_maxpool_nhwc")(_pool_case("maxpool_nhwc", ((3, 2, 1), (2, 2, 0))))
case("pool-same-nhwc", "wsc_pool_same_nhwc")(_pool_case("pool_same_nhwc", ((False, 2), (True, 1))))
case("pool-tf-nhwc", "wsc_pool_tf_nhwc")(_pool_case("pool_tf_nhwc", ((3, 2, 1), (2, 2, 0))))


@case("group-norm", "wsc_group_norm_nhwc")
def _group_norm(ctx):
    from tests import test_gpu_layers as tl

    outs = []
    rng = np.random.default_rng(3)
    # (C, G, Ctot, coff, H, W, up, Hd, Wd): the chunk boundary of the statistics, a slice of a wider buffer on the scalar and the
    # 8-channel kernels, up = 2 with a crop, up = 4
    for C, G, Ctot, coff, H, W, up, Hd, Wd in ((6, 3, 10, 3, 25, 41, 1, 25, 41), (32, 4, 192, 64, 33, 31, 1, 33, 31), (16, 2, 24, 4, 3, 5, 2, 5, 9),
                                               (16, 2, 24, 8, 3, 5, 2, 5, 9), (32, 4, 192, 64, 5, 7, 4, 17, 26), (12, 3, 16, 4, 3, 5, 2, 6, 10)):
        x, gamma, beta = tl._gn_data(rng, 2, H, W, C, G, "plain")
        for prec in PRECS.values():
            if prec == _lib.PREC_F32 and (C % 4 or Ctot % 4 or coff % 4):
                continue  # ("gn fp32 slice": WSC_ERR_INVALID)
            outs.append(tl._gn_run(ctx, x, gamma, beta, G, up, 1, Hd, Wd, Ctot, coff, prec))
    return outs


@case("gap-linear-sigmoid", "wsc_gap_linear_sigmoid")
def _gap(ctx):
    outs = []
    rng = np.random.default_rng(5)
    for npix in (5, 63):
        for F in (64, 72):
            feat = rng.normal(0, 1, (4, npix, F)).astype(np.float32)
            w = (rng.normal(0, 1, (20, F)) / np.sqrt(F)).astype(np.float32)
            b = rng.normal(0, 0.5, 20).astype(np.float32)
            f_dev = ctx.to_device(feat)
            for prec in (_lib.PREC_F16X3, _lib.PREC_BF16, _lib.PREC_F32):
                for hw, stride, bias in ((npix, 2, b), (-npix, 1, None)):
                    s_dev, shp = _lib.gap_linear_sigmoid(ctx, f_dev, 2, hw, F, w, bias, stride, prec)
                    outs.append(host(ctx, s_dev, shp))
    return outs


@case("cam-flip-add", "wsc_cam_flip_add")
def _flip_add(ctx):
    rng = np.random.default_rng(11)
    outs = []
    for h, w in ((1, 1), (3, 5), (4, 6)):
        head = rng.normal(0, 2, (4, h, w, 8)).astype(np.float32)
        c_dev, shp = _lib.cam_flip_add(ctx, ctx.to_device(head), 2, h, w, 5, 8)
        outs.append(host(ctx, c_dev, shp))
    return outs


@case("irn-edge-finish", "wsc_irn_edge_finish")
def _edge_finish(ctx):
    rng = np.random.default_rng(12)
    outs = []
    for He, We, Hd, Wd, fh, fw in ((6, 8, 6, 8, 4, 5), (8, 10, 4, 5, 4, 5), (1, 3, 2, 2, 1, 1)):
        e = rng.normal(0, 2, (4, He, We)).astype(np.float32)
        d = rng.normal(0, 3, (4, Hd, Wd, 2)).astype(np.float32)
        edge_dev, dp_dev = _lib.irn_edge_finish(ctx, ctx.to_device(e), He, We, ctx.to_device(d), Hd, Wd, 2, fh, fw, 0.375, -1.625)
        outs += [host(ctx, edge_dev, (2, fh, fw)), host(ctx, dp_dev, (2, 2, fh, fw))]
    return outs


# ---- whole nets --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cam_sd(arch):
    from oracle import cnn_ref

    if arch == "resnet50":
        return cnn_ref.make_resnet50_cam_state_dict(20, seed=0)
    if arch == "vgg16":
        return cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, 20, True, seed=1)
    if arch == "vgg16-nobn":
        return cnn_ref.make_plain_state_dict("vgg16", cnn_ref.VGG16_CFG, 20, False, seed=1)
    sd = dict(cnn_ref.make_plain_state_dict("m7", cnn_ref.M7_CFG, 20, True, seed=2))
    import torch

    sd["gradcam_weights"] = torch.from_numpy((np.random.default_rng(4).normal(0, 1, (256, 20)) / 16).astype(np.float32))
    return sd


@contextlib.contextmanager
def cam_net(ctx, arch, prec):
    """The package's own model object on the shared context: its wsc_net is created (and destroyed) inside the block."""
    from wsscam.net import m7_cam, resnet50_cam, vgg16_cam

    cls = {"resnet50": resnet50_cam.CAM, "vgg16": vgg16_cam.CAM, "vgg16-nobn": vgg16_cam.CAM, "m7": m7_cam.CAM}[arch]
    m = cls(None, "voc12", "", 20, None, precision=prec)
    m.load_state_dict(_cam_sd(arch))
    m._ctx = ctx
    try:
        yield m._ensure_net()
    finally:
        m._release_net()
        m._ctx = None


def _cam_input(B, H, W):
    return np.random.default_rng(B + H + W).normal(0, 1, (B, 2, 3, H, W)).astype(np.float32)


def _forward_cam_case(arch, prec, sizes):
    def fn(ctx):
        outs = []
        with cam_net(ctx, arch, prec) as net:
            for H, W in sizes:
                x_dev = ctx.to_device(_cam_input(2, H, W))
                h, w = net.cam_size_hw(H, W)
                # (the ResNet50 CAM net has no classifier branch: score_dev must be NULL)
                cam_dev, score_dev = out(ctx, (2, 20, h, w)), (out(ctx, (2, 20)) if arch != "resnet50" else None)
                if H == W:
                    net.forward_cam(x_dev, 2, H, cam_dev, score_dev)
                else:
                    net.forward_cam_hw(x_dev, 2, H, W, cam_dev, score_dev)
                outs.append(host(ctx, cam_dev, (2, 20, h, w)))
                if score_dev is not None:
                    outs.append(host(ctx, score_dev, (2, 20)))
        return outs
    return fn


for _arch in ("resnet50", "vgg16", "vgg16-nobn", "m7"):
    for _name in ("f16x3", "f16", "f32"):
        case("forward-cam-%s-%s" % (_arch, _name), "wsc_net_create", "wsc_net_forward_cam", "wsc_net_forward_cam_hw")(
            _forward_cam_case(_arch, PRECS[_name], ((64, 64), (65, 97))))


@functools.lru_cache(maxsize=None)
def _irn_sd(arch):
    from oracle import irn_ref

    return {"resnet50": lambda: irn_ref.make_resnet50_irn_state_dict(seed=3), "vgg16": lambda: irn_ref.make_vgg16_irn_state_dict(seed=2),
            "m7": lambda: irn_ref.make_m7_irn_state_dict(seed=4)}[arch]()


@contextlib.contextmanager
def irn_model(ctx, arch, prec=None):
    from wsscam.net import m7_irn, resnet50_irn, vgg16_irn

    if arch == "resnet50":
        m = resnet50_irn.EdgeDisplacement(None, 20, crop_size=64, stride=4, precision=prec)
    else:
        m = (vgg16_irn if arch == "vgg16" else m7_irn).EdgeDisplacement(None, "voc12", "", 20, None, crop_size=64, stride=4, precision=prec)
    m.load_state_dict(_irn_sd(arch))
    m._ctx = ctx
    try:
        m._ensure_net()
        yield m
    finally:
        m._release_net()
        m._ctx = None


def _edge_input(N, S):
    return np.random.default_rng(100 + N + S).normal(0, 1, (N, 3, S, S)).astype(np.float32)


def _forward_edge_case(arch, prec):
    def fn(ctx):
        with irn_model(ctx, arch, prec) as m:
            net = m._net
            S, B = 64, 1
            (He, We), (Hd, Wd) = net.edge_size(S)
            x_dev = ctx.to_device(_edge_input(2 * B, S))
            fh, fw = min(He, Hd) - 1, min(We, Wd) - 2
            edge_dev, dp_dev = out(ctx, (B, fh, fw)), out(ctx, (B, 2, fh, fw))
            net.forward_edge(x_dev, B, S, fh, fw, edge_dev, dp_dev)
            re_dev, rd_dev = out(ctx, (2 * B, He, We)), out(ctx, (2 * B, 2, Hd, Wd))
            net.forward_edge_raw(x_dev, 2 * B, S, re_dev, rd_dev)
            return [host(ctx, edge_dev, (B, fh, fw)), host(ctx, dp_dev, (B, 2, fh, fw)), host(ctx, re_dev, (2 * B, He, We)),
                    host(ctx, rd_dev, (2 * B, 2, Hd, Wd))]
    return fn


for _arch in ("resnet50", "vgg16", "m7"):
    for _name in ("f16x3", "f32"):
        case("forward-edge-%s-%s" % (_arch, _name), "wsc_net_create", "wsc_net_forward_edge", "wsc_net_forward_edge_raw")(
            _forward_edge_case(_arch, PRECS[_name]))


def _plain_input():
    return np.random.default_rng(21).normal(0, 1, (3, 3, 65, 65)).astype(np.float32)


def _features_case(arch):
    def fn(ctx):
        x = _plain_input()
        N, S = x.shape[0], x.shape[2]
        with cam_net(ctx, arch, _lib.PREC_F16X3) as net:
            h, F = net.cam_size(S), net.feat_channels()
            feat_dev = out(ctx, (N, h, h, F))
            net.forward_features(ctx.to_device(x), N, S, feat_dev)
            return [host(ctx, feat_dev, (N, h, h, F))]
    return fn


def _gradcam_case(arch):
    def fn(ctx):
        x = _plain_input()
        N, S = x.shape[0], x.shape[2]
        outs = []
        with cam_net(ctx, arch, _lib.PREC_F16X3) as net:
            x_dev, h = ctx.to_device(x), net.cam_size(S)
            for relu in (0, 1):
                cams_dev, score_dev = out(ctx, (N, h, h, 20)), out(ctx, (N, 20))
                net.forward_gradcam(x_dev, N, S, relu, cams_dev, score_dev)
                outs += [host(ctx, cams_dev, (N, h, h, 20)), host(ctx, score_dev, (N, 20))]
        return outs
    return fn


for _arch in ("vgg16", "m7"):
    case("forward-features-%s" % _arch, "wsc_net_forward_features")(_features_case(_arch))
    case("forward-gradcam-%s" % _arch, "wsc_net_forward_gradcam")(_gradcam_case(_arch))


@case("forward-trace-resnet50", "wsc_net_forward_trace")
def _forward_trace(ctx):
    from tests import test_gpu_net_trace as tnt

    with cam_net(ctx, "resnet50", _lib.PREC_F16X3) as net:
        plan, entries = tnt._trace(ctx, net, _edge_input(2, 64), 2, 64, 64)
        return [e for e in entries if e is not None]


# ---- dense CRF ---------------------------------------------------------------------------------------------------------------------
CRF_CFG = (1.5, 3, 40, 13, 10, 3)  # test_gpu_crf.CFGS[0] at 3 iterations


def _crf_case(H, W, M, on_chip):
    def fn(ctx):
        from tests import helpers

        rng = np.random.default_rng(H * 100 + W + M)
        cases = [helpers.synth_crf_case(rng, H, W, M) for _ in range(2)]
        B, N, Mp = 2, H * W, (M + 3) // 4 * 4
        rgb_dev = ctx.to_device(np.stack([c[0] for c in cases]))
        U = np.stack([c[1] for c in cases])
        u_dev = ctx.to_device(U)
        Upm = np.zeros((B, N, Mp), np.float32)
        Upm[:, :, :M] = np.transpose(U, (0, 2, 1))
        upm_dev = ctx.to_device(Upm)
        outs = []
        with ctx.option(_lib.OPT_CRF_GAUSS_ON_CHIP, 1 if on_chip else 0):
            for _ in range(2):  # (the second Crf of the size finds its Gaussian lattice in the context's cache)
                crf = _lib.Crf(ctx, rgb_dev, B, H, W, CRF_CFG[0], CRF_CFG[2], CRF_CFG[3])
                try:
                    q_dev, a_dev, a2_dev = out(ctx, (B, M, N)), out(ctx, (B, N), np.int32), out(ctx, (B, N), np.int32)
                    crf.inference(u_dev, M, CRF_CFG[1], CRF_CFG[4], CRF_CFG[5], q_dev, a_dev)
                    crf.inference(upm_dev, M, CRF_CFG[1], CRF_CFG[4], CRF_CFG[5], None, a2_dev, pixel_major=True)
                    outs += [host(ctx, q_dev, (B, M, N)), host(ctx, a_dev, (B, N), np.int32), host(ctx, a2_dev, (B, N), np.int32)]
                    outs += [np.asarray(v) for v in crf.lattice_sizes()]
                finally:
                    crf.close()
        return outs
    return fn


_CRF_ENTRIES = ("wsc_crf_create", "wsc_crf_inference", "wsc_crf_inference_pm", "wsc_crf_lattice_sizes")
for _hw, _on in (((47, 61), True), ((47, 61), False), ((1, 37), True), ((3, 5), True)):
    case("crf-%dx%d-M5-%s" % (_hw + ("on-chip" if _on else "three-pass",)), *_CRF_ENTRIES, fresh=True)(_crf_case(_hw[0], _hw[1], 5, _on))


@case("crf-v-ragged", "wsc_crf_v_create", "wsc_crf_v_inference", fresh=True)
def _crf_v(ctx):
    from tests import helpers

    rng = np.random.default_rng(41)
    sizes, Ms = [(21, 27), (47, 61)], [3, 5]
    cases = [helpers.synth_crf_case(rng, h, w, m) for (h, w), m in zip(sizes, Ms)]
    rgbs = [ctx.to_device(c[0]) for c in cases]
    us = [ctx.to_device(c[1]) for c in cases]
    qs = [out(ctx, (m, h * w)) for (h, w), m in zip(sizes, Ms)]
    ams = [out(ctx, (h * w,), np.int32) for h, w in sizes]
    crf = _lib.CrfV(ctx, rgbs, sizes, CRF_CFG[0], CRF_CFG[2], CRF_CFG[3])
    try:
        crf.inference(us, Ms, CRF_CFG[1], CRF_CFG[4], CRF_CFG[5], qs, ams)
        return [host(ctx, q, (m, h * w)) for q, (h, w), m in zip(qs, sizes, Ms)] + [host(ctx, a, (h * w,), np.int32) for a, (h, w) in zip(ams, sizes)]
    finally:
        crf.close()


# ---- random walk -------------------------------------------------------------------------------------------------------------------
RW_SHAPES = [(2, 15, 20), (7, 33, 47), (1, 1, 1)]


def _rw_inputs():
    rng = np.random.default_rng(5)
    xs = [rng.random(s).astype(np.float32) for s in RW_SHAPES]
    es = [(rng.random(s[1:]) ** 2).astype(np.float32) for s in RW_SHAPES]
    return xs, es


def _rw_upload(ctx):
    xs, es = _rw_inputs()
    return ctx.to_device(np.concatenate([x.ravel() for x in xs])), ctx.to_device(np.concatenate([e.ravel() for e in es]))


def _rw_run(ctx, x_dev, e_dev, rw_dev=None, n_steps=8):
    from wsscam.misc.indexing import PathIndex

    dirs, start, yx = PathIndex(5).device_tables()
    rw_dev = _lib.rw_propagate_batch(ctx, x_dev, e_dev, [s[0] for s in RW_SHAPES], [s[1] for s in RW_SHAPES], [s[2] for s in RW_SHAPES], dirs,
                                     start, yx, 10.0, n_steps, rw_dev)
    return rw_dev, sum(int(np.prod(s)) for s in RW_SHAPES)


def _rw_call(ctx):
    return _rw_run(ctx, *_rw_upload(ctx))


def _rw_batch_case(tiled):
    def fn(ctx):
        with ctx.option(_lib.OPT_RW_TILED, tiled):
            rw_dev, n = _rw_call(ctx)
            return [host(ctx, rw_dev, (n,))]
    return fn


case("rw-propagate-batch-tiled", "wsc_rw_propagate_batch")(_rw_batch_case(1))
case("rw-propagate-batch-flat", "wsc_rw_propagate_batch")(_rw_batch_case(0))


@case("rw-propagate", "wsc_rw_propagate")
def _rw(ctx):
    from wsscam.misc.indexing import PathIndex

    xs, es = _rw_inputs()
    dirs, start, yx = PathIndex(5).device_tables()
    K, h, w = RW_SHAPES[0]
    rw_dev = _lib.rw_propagate(ctx, ctx.to_device(xs[0]), ctx.to_device(es[0]), K, h, w, dirs, start, yx, 10.0, 8)
    return [host(ctx, rw_dev, (K, h, w))]


# ---- SEC / DSRG: forward, tape, training step -----------------------------------------------------------------------------------
def _seg_forward_case(method, hw, prec):
    def fn(ctx):
        from tests import deeplab_ref as dref
        from wsscam import secdsrg

        weights, x = dref.thin_case(method, 5, hw)
        net = secdsrg.SegNet(method, weights, 5, precision=prec, ctx=ctx)
        try:
            prob, fc8 = net.forward(x, want_fc8=True)                                        # wsc_net_forward_seg
            outs = [prob, fc8]
            for dropout in (None, (0.5, (9 << 32) + 7, 3)):                                    # ..._seg_tape / ..._seg_train
                p, f, tape = net.forward_dev(x, want_fc8=True, keep=True, dropout=dropout)
                with p, f, tape:
                    flat = tape.to_host()
                    B = x.shape[0]
                    outs += [p.to_host(), f.to_host()] + [flat[e["offset"]:e["offset"] + B * e["Ho"] * e["Wo"] * e["C"]] for e in tape.entries]
            return outs
        finally:
            net.close()
    return fn


for _m in ("SEC", "DSRG"):
    for _hw in ((65, 65), (64, 48)):
        for _name in ("f16x3", "f32"):
            case("forward-seg-%s-%dx%d-%s" % (_m, _hw[0], _hw[1], _name), "wsc_net_create", "wsc_net_forward_seg", "wsc_net_forward_seg_tape",
                 "wsc_net_forward_seg_train")(_seg_forward_case(_m, _hw, PRECS[_name]))


def _seg_trainer_case(method, drop_prob):
    def fn(ctx):
        from tests import test_gpu_seg_dropout as tsd
        from wsscam import secdsrg

        weights, x, cues, tags = tsd._step_case(method)
        tr = secdsrg.SegTrainer(method, weights, 5, ctx=ctx, drop_prob=drop_prob, seed=(9 << 32) + 2024)
        try:
            outs = []
            for _ in range(2):  # (the second step runs on the weights wsc_net_seg_load_params repacked)
                losses, new_cues = tr.step(x, cues, tags, tsd.MEAN, tsd.CRF_CFG)
                with new_cues:
                    outs += [np.array([losses[k] for k in sorted(losses)], np.float64), new_cues.to_host()]
                outs += [tr.params.to_host(), tr.mom.to_host(), tr.accum.to_host()]
            return outs
        finally:
            tr.close()
    return fn


_TRAIN_COMMON = ("wsc_seg_grad_create", "wsc_seg_crf_image_u8", "wsc_seg_unary_nhwc", "wsc_seg_crf_logprob", "wsc_seg_loss",
                 "wsc_seg_sgd_accumulate", "wsc_seg_sgd_apply", "wsc_net_seg_load_params", "wsc_crf_create", "wsc_crf_inference")
for _m in ("SEC", "DSRG"):
    _grow = ("wsc_dsrg_seed_grow",) if _m == "DSRG" else ()
    case("seg-trainer-%s" % _m, "wsc_net_forward_seg_tape", "wsc_net_backward_seg", *_TRAIN_COMMON, *_grow)(_seg_trainer_case(_m, 0.0))
    case("seg-trainer-%s-dropout" % _m, "wsc_net_forward_seg_train", "wsc_net_backward_seg_drop", *_TRAIN_COMMON, *_grow)(_seg_trainer_case(_m, 0.5))


# ---- the direct entries of the backward passes -------------------------------------------------------------------------------------
@case("conv2d-wgrad-nhwc", "wsc_conv2d_wgrad_nhwc")
def _wgrad_direct(ctx):
    from tests import test_gpu_seg_grad as tsg

    outs = []
    for c in tsg.WGRAD_SMALL_CASES:
        N, H, W, Cin, Cout, k, dil, splits = c
        rng = np.random.default_rng(sum(c))
        x = np.maximum(rng.standard_normal((N, H, W, Cin)), -0.5).astype(np.float32)
        dz = (1e-3 * rng.standard_normal((N, H, W, Cout))).astype(np.float32)
        dw, db = out(ctx, (k, k, Cin, Cout)), out(ctx, (Cout,))
        _lib.conv2d_wgrad_nhwc(ctx, ctx.to_device(x), ctx.to_device(dz), N, H, W, Cin, Cout, k, dil, splits, dw, db)
        outs += [host(ctx, dw, (k, k, Cin, Cout)), host(ctx, db, (Cout,))]
    return outs


@case("conv2d-dgrad-nhwc", "wsc_conv2d_dgrad_nhwc")
def _dgrad_direct(ctx):
    from tests import test_gpu_seg_grad as tsg

    outs = []
    for c in tsg.DGRAD_SMALL_CASES:
        N, H, W, Cin, Cout, k, dil = c
        rng = np.random.default_rng(sum(c) + 1)
        dz = (1e-3 * rng.standard_normal((N, H, W, Cout))).astype(np.float32)
        w = rng.standard_normal((k, k, Cin, Cout)).astype(np.float32)
        dx = out(ctx, (N, H, W, Cin))
        _lib.conv2d_dgrad_nhwc(ctx, ctx.to_device(dz), w, N, H, W, Cin, Cout, k, dil, dx)
        outs.append(host(ctx, dx, (N, H, W, Cin)))
    return outs


@case("relu-bias-grad", "wsc_relu_bias_grad", "wsc_relu_bias_grad_scaled")
def _relu_bias_grad_direct(ctx):
    from tests import test_gpu_seg_grad as tsg

    outs = []
    for M, C, mask in ((70, 64, True), (1, 64, True), (96, 2, False), (3069, 192, True)):
        rng = np.random.default_rng(M + C)
        y = tsg._relu_like(rng, (M, C))
        dy = (1e-3 * rng.standard_normal((M, C))).astype(np.float32)
        y_dev, dy_dev = ctx.to_device(y), ctx.to_device(dy)
        for scale in (None, 2.0):
            dz, db = out(ctx, (M, C)), out(ctx, (C,))
            if scale is None:
                _lib.relu_bias_grad(ctx, y_dev if mask else None, dy_dev, M, C, dz, db)
            else:
                _lib.relu_bias_grad_scaled(ctx, y_dev if mask else None, dy_dev, M, C, scale, dz, db)
            outs += [host(ctx, dz, (M, C)), host(ctx, db, (C,))]
    return outs


@case("pool-same-grad-nhwc", "wsc_pool_same_grad_nhwc")
def _pool_grad_direct(ctx):
    from tests import test_gpu_seg_grad as tsg

    outs = []
    for avg, stride, shape in ((0, 2, (2, 9, 9, 64)), (0, 1, (1, 1, 7, 64)), (1, 1, (2, 8, 6, 64)), (0, 2, (1, 2, 2, 64)), (1, 1, (1, 1, 1, 64))):
        N, H, W, C = shape
        rng = np.random.default_rng(sum(shape) + 10 * stride + avg)
        x = tsg._relu_like(rng, shape)
        Ho, Wo = -(-H // stride), -(-W // stride)
        dy = (1e-3 * rng.standard_normal((N, Ho, Wo, C))).astype(np.float32)
        dx = out(ctx, shape)
        _lib.pool_same_grad_nhwc(ctx, ctx.to_device(x), ctx.to_device(dy), N, H, W, C, avg, stride, dx)
        outs.append(host(ctx, dx, shape))
    return outs


@case("relu-upsample-grad-nhwc", "wsc_relu_upsample_grad_nhwc")
def _up_grad_direct(ctx):
    from tests import test_gpu_irn_grad as tig

    outs = []
    for c in ((1, 1, 1, 32, 4, 3, 2, 192, 96), (1, 1, 7, 64, 2, 2, 14, 448, 0), (2, 5, 5, 30, 2, 9, 9, 101, 7), (3, 6, 4, 64, 1, 6, 4, 448, 0)):
        N, H, W, C, up, Hd, Wd, Ctot, coff = c
        rng = np.random.default_rng(sum(c))
        cat = tig._relu_like(rng, (N, Hd, Wd, Ctot))
        dcat = rng.standard_normal((N, Hd, Wd, Ctot)).astype(np.float32)
        dy = out(ctx, (N, H, W, C))
        _lib.relu_upsample_grad_nhwc(ctx, ctx.to_device(dcat), ctx.to_device(cat), N, H, W, C, up, Hd, Wd, Ctot, coff, dy)
        outs.append(host(ctx, dy, (N, H, W, C)))
    return outs


@case("group-norm-grad-nhwc", "wsc_group_norm_grad_nhwc")
def _gn_grad_direct(ctx):
    from tests import irn_grad_ref as gref

    outs = []
    for c in ((1, 1, 1, 32, 4), (2, 5, 3, 32, 4), (2, 7, 5, 6, 2), (1, 33, 32, 32, 4)):
        N, H, W, C, G = c
        z, dy, gamma = gref.gn_case(c, 5)
        dz, dg, db = out(ctx, (N, H, W, C)), out(ctx, (C,)), out(ctx, (C,))
        _lib.group_norm_grad_nhwc(ctx, ctx.to_device(z), ctx.to_device(dy), N, H, W, C, gamma, G, gref.EPS, dz, dg, db)
        outs += [host(ctx, dz, (N, H, W, C)), host(ctx, dg, (C,)), host(ctx, db, (C,))]
    return outs


@case("channel-mean-nchw", "wsc_channel_mean_nchw")
def _channel_mean_direct(ctx):
    outs = []
    for shape, sub in (((3, 2, 17, 17), None), ((1, 2, 1, 1), [0.375, -1e-3]), ((2, 2, 128, 128), [0.375, -1e-3])):
        x = (np.random.default_rng(sum(shape)).standard_normal(shape) * 3).astype(np.float32)
        m = out(ctx, (shape[1],), np.float64)
        _lib.channel_mean_nchw(ctx, ctx.to_device(x), *shape, m, sub=sub)
        outs.append(host(ctx, m, (shape[1],), np.float64))
    return outs


@case("irn-backward-edge-resnet50", "wsc_net_forward_edge_tape", "wsc_net_edge_tape_plan", "wsc_irn_grad_create", "wsc_net_backward_edge")
def _backward_edge(ctx):
    """the smallest of test_gpu_irn_grad.E2E: resnet50, S = 64, N = 1, f16x3"""
    from wsscam.secdsrg import DeviceMaps

    with irn_model(ctx, "resnet50", _lib.PREC_F16X3) as m:
        N, S = 1, 64
        edge, dp, tape = m.forward_train_dev(_edge_input(N, S), keep=True)
        with edge, dp, tape:
            rng = np.random.default_rng(S + N)
            d_edge = (1e-3 * rng.standard_normal(edge.shape)).astype(np.float32)
            d_dp = (1e-3 * rng.standard_normal(dp.shape)).astype(np.float32)
            with DeviceMaps.from_host(ctx, d_edge) as de, DeviceMaps.from_host(ctx, d_dp) as dd:
                g = m.backward_dev(tape, de, dd)
                try:
                    # (the tape's entries start on 256-byte lines: the floats between them are the caller's)
                    return [edge.to_host(), dp.to_host(), g.maps.to_host()] + [tape.entry(e["name"]) for e in tape.entries]
                finally:
                    g.maps.free()


@case("irn-trainer-vgg16", "wsc_net_forward_edge_tape", "wsc_irn_aff_loss", "wsc_net_backward_edge", "wsc_irn_sgd_step", "wsc_net_irn_load_params",
      "wsc_irn_grad_create")
def _irn_trainer(ctx):
    from tests import test_gpu_irn_sgd as tis
    from wsscam import irn_train
    from wsscam.misc.indexing import PathIndex

    x, label = tis._trainer_case()
    with irn_model(ctx, "vgg16", _lib.PREC_F16X3) as m:
        tr = irn_train.IrnTrainer(m, PathIndex(5), tis.LR, tis.WD, tis.MAX_STEP, power=tis.POWER)
        try:
            outs = []
            for _ in range(2):
                losses = tr.step(x, label)
                outs += [np.array([losses[k] for k in sorted(losses)], np.float64), tr.params.to_host(), tr.mom.to_host()]
            return outs
        finally:
            tr.close()


# ---- losses and label growing ------------------------------------------------------------------------------------------------------
def _loss_maps():
    rng = np.random.default_rng(13)
    B, h, w, C = 3, 7, 5, 5  # test_gpu_seg_loss.SHAPES[0]
    logits = rng.normal(0, 2, (B, h, w, C))
    prob = (np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)).astype(np.float32)
    crf = np.log(np.clip(prob[..., ::-1] * 0.9 + 0.02, 1e-4, 1)).astype(np.float32)
    cues = (rng.random((B, h, w, C)) < 0.2).astype(np.float32)
    labels = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 1], [1, 0, 0, 0, 1]], np.float32)
    return prob, crf, cues, labels


def _seg_loss_case(method):
    def fn(ctx):
        from wsscam import secdsrg

        prob, crf, cues, labels = _loss_maps()
        outs = []
        for want in ("fc8", "prob"):
            losses, grad = secdsrg.SegLoss(method, prob.shape[3], ctx=ctx)(prob, crf, cues, labels=labels, want_grad=want)
            with grad:
                outs += [np.array([losses[k] for k in sorted(losses)], np.float64), grad.to_host()]
        return outs
    return fn


for _m in ("SEC", "DSRG"):
    case("seg-loss-%s" % _m, "wsc_seg_loss")(_seg_loss_case(_m))


@case("irn-aff-loss", "wsc_irn_aff_loss")
def _irn_aff_loss(ctx):
    from tests import irn_loss_ref, test_gpu_irn_loss as til

    case1 = irn_loss_ref.CASES[1]
    edge, dp, label = irn_loss_ref.make_case(case1)
    return list(til.run(ctx, edge, dp, label, case1[0]))


@case("dsrg-seed-grow", "wsc_dsrg_seed_grow")
def _dsrg_grow(ctx):
    prob, _, cues, labels = _loss_maps()
    B, h, w, C = prob.shape
    grown = out(ctx, (B, h, w, C))
    _lib.dsrg_seed_grow(ctx, ctx.to_device(labels), ctx.to_device(cues), ctx.to_device(prob), B, h, w, C, grown)
    return [host(ctx, grown, (B, h, w, C))]


@case("seg-dropout-f32", "wsc_seg_dropout_f32")
def _seg_dropout(ctx):
    x = np.random.default_rng(14).standard_normal(1003).astype(np.float32)
    y, keep = out(ctx, (1003,)), out(ctx, (1003,), np.uint8)
    _lib.seg_dropout_f32(ctx, ctx.to_device(x), 1003, (1 << 32) - 5, 0.5, (9 << 32) + 1, 2, 3, y, keep)
    return [host(ctx, y, (1003,)), host(ctx, keep, (1003,), np.uint8)]


@case("cue-seeds", "wsc_cue_seeds")
def _cue_seeds(ctx):
    rng = np.random.default_rng(17)
    outs = []
    B, C, Cb, H, W = 2, 5, 2, 41, 37
    fg = np.maximum(rng.normal(0.2, 0.5, (B, C, H, W)), 0).astype(np.float32)
    bg = np.maximum(rng.normal(0.2, 0.5, (B, Cb, H, W)), 0).astype(np.float32)
    fg_dev, bg_dev = ctx.to_device(fg), ctx.to_device(bg)
    for use_bg, per_image in ((True, False), (False, True)):
        L = C + (1 if use_bg else 0)
        lab, area = out(ctx, (B, H * W), np.uint8), out(ctx, (B, L), np.int32)
        _lib.cue_seeds(ctx, fg_dev, bg_dev if use_bg else None, B, C, Cb if use_bg else 0, H, W, 0.2, lab, area, per_image_max=per_image)
        outs += [host(ctx, lab, (B, H * W), np.uint8), host(ctx, area, (B, L), np.int32)]
    return outs


@case("cue-maps", "wsc_cue_maps")
def _cue_maps(ctx):
    rng = np.random.default_rng(18)
    B, h, C_all, chan, S = 2, 8, 20, [0, 2, 5, 19], 41
    cams = rng.normal(0.1, 1.0, (B, h, h, C_all)).astype(np.float32)
    gate = (rng.random((B, len(chan))) > 0.3).astype(np.float32)
    maps = out(ctx, (B, len(chan), S, S))
    _lib.cue_maps(ctx, ctx.to_device(cams), B, h, h, C_all, chan, ctx.to_device(gate), S, maps)
    return [host(ctx, maps, (B, len(chan), S, S))]


# ---- CAM / label tails -------------------------------------------------------------------------------------------------------------
CAM_SIZES = [(37, 50), (64, 41), (1, 7)]


def _cam_maps():
    return np.maximum(np.random.default_rng(21).normal(0.3, 1.0, (3, 20, 21, 21)), 0).astype(np.float32)


def _cam_gt(ctx):
    rng = np.random.default_rng(22)
    gts = [rng.integers(0, 21, sz).astype(np.uint8) for sz in CAM_SIZES]
    for g in gts:
        g[rng.random(g.shape) < 0.1] = 255
    return ctx.to_device(np.concatenate([g.ravel() for g in gts])), sum(a * b for a, b in CAM_SIZES)


@case("cam-postprocess+eval-confusion", "wsc_cam_postprocess", "wsc_cam_eval_confusion")
def _cam_postprocess(ctx):
    B, C, h = 3, 20, 21
    keys = [[2, 9, 19], [], [0]]
    s_dev, h_dev, s_off, h_off, shapes = _lib.cam_postprocess(ctx, ctx.to_device(_cam_maps()), B, C, h, h, CAM_SIZES, keys)
    n_s, n_h = sum(k * a * b for k, a, b, _, _ in shapes), sum(k * a * b for k, _, _, a, b in shapes)
    gt_dev, n_pix = _cam_gt(ctx)
    conf, pred = ctx.to_device(np.zeros((21, 21), np.int64)), out(ctx, (n_pix,), np.uint8)
    _lib.cam_eval_confusion(ctx, h_dev, CAM_SIZES, keys, h_off, 0.15, gt_dev, 21, conf, pred)
    return [host(ctx, s_dev, (n_s,)), host(ctx, h_dev, (n_h,)), host(ctx, conf, (21, 21), np.int64), host(ctx, pred, (n_pix,), np.uint8)]


@case("cam-eval-confusion-nn", "wsc_cam_eval_confusion_nn")
def _cam_confusion_nn(ctx):
    """the maps at the strided size (host-made, every key list non-empty), the ground truth at the image's"""
    rng = np.random.default_rng(24)
    keys = [[2, 9, 19], [4], [0, 1]]
    src = [((a - 1) // 4 + 1, (b - 1) // 4 + 1) for a, b in CAM_SIZES]
    maps = [rng.random((len(k), a, b), dtype=np.float32) for k, (a, b) in zip(keys, src)]
    off = np.concatenate([[0], np.cumsum([m.size for m in maps])])[:-1]
    gt_dev, n_pix = _cam_gt(ctx)
    conf, pred = ctx.to_device(np.zeros((21, 21), np.int64)), out(ctx, (n_pix,), np.uint8)
    _lib.cam_eval_confusion_nn(ctx, ctx.to_device(np.concatenate([m.ravel() for m in maps])), src, CAM_SIZES, keys, off, gt_dev, 21, conf, pred)
    return [host(ctx, conf, (21, 21), np.int64), host(ctx, pred, (n_pix,), np.uint8)]


@case("label-confusion-nn", "wsc_label_confusion_nn")
def _label_confusion_nn(ctx):
    rng = np.random.default_rng(25)
    src = [(11, 9), (5, 7), (3, 3)]
    labs = [rng.integers(0, 21, sz).astype(np.int32) for sz in src]
    off = np.concatenate([[0], np.cumsum([l.size for l in labs])])[:-1]
    gt_dev, n_pix = _cam_gt(ctx)
    conf, pred = ctx.to_device(np.zeros((21, 21), np.int64)), out(ctx, (n_pix,), np.uint8)
    _lib.label_confusion_nn(ctx, ctx.to_device(np.concatenate([l.ravel() for l in labs])), src, CAM_SIZES, off, gt_dev, 21, conf, pred)
    return [host(ctx, conf, (21, 21), np.int64), host(ctx, pred, (n_pix,), np.uint8)]


def _cam_unary_case(pm):
    def fn(ctx):
        B, C, h, H0, W0 = 3, 20, 21, 47, 61
        Mp = (C + 1 + 3) // 4 * 4 if pm else C + 1
        u = out(ctx, (B, Mp, H0 * W0))
        _lib.cam_unary(ctx, ctx.to_device(_cam_maps()), B, C, h, h, H0, W0, 0.15, u, pixel_major=pm)
        # (the whole buffer: the pixel-major form writes its padding classes too)
        return [host(ctx, u, (B, H0 * W0, Mp) if pm else (B, Mp, H0 * W0))]
    return fn


case("cam-unary", "wsc_cam_unary")(_cam_unary_case(False))
case("cam-unary-pm", "wsc_cam_unary_pm")(_cam_unary_case(True))


@case("unary-from-maps", "wsc_unary_from_maps")
def _unary_from_maps(ctx):
    maps = np.random.default_rng(26).random((2, 4, 47 * 59), dtype=np.float32)
    u = out(ctx, (2, 5, 47 * 59))
    _lib.unary_from_maps(ctx, ctx.to_device(maps), 2, 4, 47 * 59, 0.15, u)
    return [host(ctx, u, (2, 5, 47 * 59))]


@case("cam-sum-scales", "wsc_cam_sum_scales")
def _cam_sum_scales(ctx):
    sc = np.random.default_rng(27).normal(0, 1, (6, 1001)).astype(np.float32)
    o = out(ctx, (2, 1001))
    _lib.cam_sum_scales(ctx, ctx.to_device(sc), 2, 3, 1001, o)
    return [host(ctx, o, (2, 1001))]


@case("bilinear-resize", "wsc_bilinear_resize")
def _bilinear_resize(ctx):
    x = np.random.default_rng(28).random((3, 50, 73), dtype=np.float32)
    outs = []
    for size in ((8, 12), (77, 101)):
        o = out(ctx, (3,) + size)
        _lib.bilinear_resize(ctx, ctx.to_device(x), 3, 50, 73, o, size[0], size[1])
        outs.append(host(ctx, o, (3,) + size))
    return outs


@case("sem-seg-finish", "wsc_sem_seg_finish")
def _sem_seg_finish(ctx):
    from tests import test_gpu_label_tail as tlt

    outs = []
    images = tlt._ragged_images()
    keys = [tlt._keys_for(b, rw.shape[0]) for b, (rw, _, _) in enumerate(images)]
    for has_bg in (True, False):
        outs += tlt._finish(ctx, images, keys if has_bg else [k[1:] for k in keys], has_bg, tlt.BG_THRES)
    return outs


@case("label-unary-from-cam", "wsc_label_unary_from_cam")
def _label_unary_from_cam(ctx):
    from tests import test_gpu_label_tail as tlt

    outs = []
    for shape in tlt.UNARY_SHAPES[:3]:
        outs += list(tlt._label_unary(ctx, tlt._unary_inputs(*shape), True))
    return outs


@case("ir-label-combine", "wsc_ir_label_combine")
def _ir_label_combine(ctx):
    from tests import test_gpu_label_tail as tlt

    outs = []
    for (B, M, N), voc in (((3, 4, 47 * 59), True), ((3, 3, 1), False)):
        k, fg, bg = tlt._combine_inputs(B, M, N, voc, B * 7 + M)
        c = out(ctx, (B, N), np.uint8)
        _lib.ir_label_combine(ctx, ctx.to_device(fg), ctx.to_device(bg) if voc else None, k, N, c)
        outs.append(host(ctx, c, (B, N), np.uint8))
    return outs


# ---- HistoSegNet tail (B = 2, S = 57) ----------------------------------------------------------------------------------------------
HSN_B, HSN_S = 2, 57


def _hsn_images():
    from tests import test_gpu_hsn as th

    rng = np.random.default_rng(3)
    raw = np.stack([th._adp_like(rng, HSN_S, HSN_S) for _ in range(HSN_B)])
    raw[1, 20:40, 10:50] = 252
    return raw


@case("hsn-gradcam-post", "wsc_hsn_gradcam_post")
def _hsn_gradcam_post(ctx):
    rng = np.random.default_rng(31)
    B, S, h, C = HSN_B, HSN_S, 10, 7
    cams = rng.normal(0.1, 1.0, (B, h, h, C)).astype(np.float32)
    gate = (rng.random((B, C)) * (rng.random((B, C)) > 0.4)).astype(np.float32)
    o = out(ctx, (B, C, S, S))
    _lib.hsn_gradcam_post(ctx, ctx.to_device(cams), B, h, h, C, S, ctx.to_device(gate), o)
    return [host(ctx, o, (B, C, S, S))]


def _hsn_background_case(out_hw):
    def fn(ctx):
        B, S = HSN_B, HSN_S
        n = S * S if out_hw is None else out_hw[0] * out_hw[1]
        bg_dev = out(ctx, (B, n), np.float64)
        _lib.hsn_background(ctx, ctx.to_device(_hsn_images()), B, S, S, bg_dev, out_hw=out_hw)
        return [host(ctx, bg_dev, (B, n), np.float64)]
    return fn


case("hsn-background", "wsc_hsn_background")(_hsn_background_case(None))
case("hsn-background-resized", "wsc_hsn_background")(_hsn_background_case((14, 14)))  # (Ho != H: the resize of the background)


def _hsn_cs_case(htt):
    def fn(ctx):
        from wsscam.hsn import demo as hsn_demo
        from wsscam.hsn import utilities as hsn

        B, S = HSN_B, HSN_S
        N = S * S
        ac = hsn_demo.ADPClasses()
        C_all = len(ac.classes["all"])
        Hm = np.maximum(np.random.default_rng(32).normal(0.0, 0.4, (B, C_all, N)), 0).astype(np.float32)
        Hm[0, 5] = 0
        # the background activation as wsc_hsn_background forms it, from the host here: this case is about the two entries below
        bg = np.random.default_rng(33).random((B, N)) * 0.75
        adipose_all = [i for i, x in enumerate(ac.classes["all"]) if x in ["A.W", "A.B", "A.M"]]
        valid = ac.classes["valid_" + htt]
        Cv = len(valid)
        src_of = [-1] * Cv
        for v, a in zip(ac.classinds[htt + "2valid"], ac.classinds["all2" + htt]):
            src_of[v] = a
        bg_ind, other_ind, ex = hsn._htt_tables(valid, htt == "func")
        cs_dev, y_dev, mass_dev = out(ctx, (B, Cv, N)), out(ctx, (B, Cv, N)), out(ctx, (B, Cv), np.uint32)
        _lib.hsn_cs_gradcam(ctx, ctx.to_device(Hm), B, C_all, N, ctx.to_device(bg), src_of, bg_ind, other_ind, ex,
                            adipose_all if htt == "func" else None, cs_dev, y_dev, mass_dev)
        mass = host(ctx, mass_dev, (B, Cv), np.uint32)
        keep = np.nonzero(mass[1])[0]
        assert len(keep) > 0
        u_dev = out(ctx, (len(keep), N))
        _lib.hsn_gather_unary(ctx, cs_dev, [(1 * Cv + int(c)) * N for c in keep], N, u_dev)
        return [host(ctx, cs_dev, (B, Cv, N)), host(ctx, y_dev, (B, Cv, N)), mass, host(ctx, u_dev, (len(keep), N))]
    return fn


for _htt in ("morph", "func"):
    case("hsn-cs-gradcam+gather-unary-%s" % _htt, "wsc_hsn_cs_gradcam", "wsc_hsn_gather_unary")(_hsn_cs_case(_htt))


@case("hsn-voc-background", "wsc_hsn_voc_background")
def _hsn_voc_background(ctx):
    B, N = HSN_B, HSN_S * HSN_S
    Hbg = (np.random.default_rng(34).random((B, 4, N)) ** 2).astype(np.float32)
    y = ctx.to_device(np.full((B, 3, N), -7.0, np.float32))  # (channel 0 is written, the others are the caller's)
    _lib.hsn_voc_background(ctx, ctx.to_device(Hbg), B, 4, N, y, 3)
    return [host(ctx, y, (B, 3, N))]


@case("hsn-class-mass", "wsc_hsn_class_mass")
def _hsn_class_mass(ctx):
    B, N = HSN_B, HSN_S * HSN_S
    maps = (np.random.default_rng(35).random((B * 4, N)) ** 2).astype(np.float32)
    maps[3] = 0
    mass_dev = out(ctx, (B * 4,), np.uint32)
    _lib.hsn_class_mass(ctx, ctx.to_device(maps), B * 4, N, mass_dev)
    return [host(ctx, mass_dev, (B * 4,), np.uint32)]


@case("cam-adp-modify", "wsc_cam_adp_modify")
def _cam_adp_modify(ctx):
    rng = np.random.default_rng(36)
    B, n_sc, Cc, hw = HSN_B, 2, 9, 14 * 14
    cam = np.maximum(rng.normal(0.2, 0.5, (B, n_sc, Cc, hw)), 0).astype(np.float32)
    bgs = rng.random((B, n_sc, hw))
    cam_dev, bgs_dev = ctx.to_device(cam), ctx.to_device(bgs)
    outs = []
    for mode, use, exc in ((0, [0, 1, 2, 3, 4], None), (1, [5, 6, 7], [5, 6])):
        n_out = len(use) + 1 + mode
        o = out(ctx, (B, n_out, hw))
        assert _lib.cam_adp_modify(ctx, cam_dev, B, n_sc, Cc, hw, bgs_dev, mode, use, [2, 3, 4], exc, o) == n_out
        outs.append(host(ctx, o, (B, n_out, hw)))
    return outs


# ---- SEC / DSRG prediction tail and the batch builders -----------------------------------------------------------------------------
SEG_MEAN = np.array([104.00698793, 116.66876762, 122.67891434], np.float32)


def _seg_ragged():
    rng = np.random.default_rng(23)
    C, src, dst = 5, [(9, 9), (6, 8)], [(21, 27), (47, 61)]
    probs = [rng.dirichlet(np.ones(C), s).astype(np.float32) for s in src]
    return C, src, dst, probs, np.concatenate([[0], np.cumsum([p.size for p in probs])])[:-1]


@case("seg-unary-nhwc", "wsc_seg_unary_nhwc")
def _seg_unary(ctx):
    C, src, dst, probs, p_off = _seg_ragged()
    d_off = np.concatenate([[0], np.cumsum([C * a * b for a, b in dst])])
    u = out(ctx, (int(d_off[-1]),))
    _lib.seg_unary_nhwc(ctx, ctx.to_device(np.concatenate([p.ravel() for p in probs])), C, src, dst, p_off, d_off[:-1], u)
    return [host(ctx, u, (int(d_off[-1]),))]


@case("seg-resize-argmax", "wsc_seg_resize_argmax")
def _seg_resize_argmax(ctx):
    C, src, dst, probs, p_off = _seg_ragged()
    q = [np.ascontiguousarray(np.transpose(p, (2, 0, 1))) for p in probs]  # class-major marginals
    l_off = np.concatenate([[0], np.cumsum([a * b for a, b in dst])])
    lab = out(ctx, (int(l_off[-1]),), np.int32)
    _lib.seg_resize_argmax(ctx, ctx.to_device(np.concatenate([v.ravel() for v in q])), C, src, dst, p_off, l_off[:-1], lab)
    return [host(ctx, lab, (int(l_off[-1]),), np.int32)]


@case("seg-preprocess-u8", "wsc_seg_preprocess_u8")
def _seg_preprocess(ctx):
    rng = np.random.default_rng(37)
    imgs = [rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8) for hh, ww in ((7, 5), (33, 41), (50, 23))]
    i_off = np.concatenate([[0], np.cumsum([im.size for im in imgs])])[:-1]
    x = out(ctx, (3, 33, 31, 3))
    _lib.seg_preprocess_u8(ctx, ctx.to_device(np.concatenate([im.ravel() for im in imgs])), [im.shape[:2] for im in imgs], i_off, SEG_MEAN,
                           (33, 31), x)
    return [host(ctx, x, (3, 33, 31, 3))]


@case("seg-crf-image-u8", "wsc_seg_crf_image_u8")
def _seg_crf_image(ctx):
    x = np.random.default_rng(38).uniform(-125.0, 150.0, (3, 33, 31, 3)).astype(np.float32)
    img8 = out(ctx, (3, 9, 8, 3), np.uint8)
    _lib.seg_crf_image_u8(ctx, ctx.to_device(x), 3, 33, 31, SEG_MEAN, (9, 8), img8)
    return [host(ctx, img8, (3, 9, 8, 3), np.uint8)]


@case("seg-planes-from-nhwc", "wsc_seg_planes_from_nhwc")
def _seg_planes(ctx):
    qq = np.random.default_rng(39).dirichlet(np.ones(5), (2, 81)).astype(np.float32)  # [B][n][C]
    planes = out(ctx, (2, 5, 81))
    _lib.seg_planes_from_nhwc(ctx, ctx.to_device(qq), 2, 5, 81, planes)
    return [host(ctx, planes, (2, 5, 81))]


@case("seg-crf-logprob", "wsc_seg_crf_logprob")
def _seg_crf_logprob(ctx):
    q = np.ascontiguousarray(np.transpose(np.random.default_rng(40).dirichlet(np.ones(5), (2, 81)), (0, 2, 1))).astype(np.float32)  # [B][C][n]
    logp = out(ctx, (2, 81, 5))
    _lib.seg_crf_logprob(ctx, ctx.to_device(q), 2, 5, 81, 1e-4, logp)
    return [host(ctx, logp, (2, 81, 5))]


@case("fc8-softmax", "wsc_fc8_softmax")
def _fc8_softmax(ctx):
    rng = np.random.default_rng(41)
    fc8 = [ctx.to_device(rng.normal(0, 2, (163, 5)).astype(np.float32)) for _ in range(4)]
    outs = []
    for n_in in (1, 4):
        prob, ssum = out(ctx, (163, 5)), out(ctx, (163, 5))
        _lib.fc8_softmax(ctx, fc8[:n_in], 163, 5, prob, sum_dev=ssum if n_in > 1 else None)
        outs.append(host(ctx, prob, (163, 5)))
        if n_in > 1:
            outs.append(host(ctx, ssum, (163, 5)))
    return outs


@case("resize-bilinear-tf", "wsc_resize_bilinear_tf")
def _resize_bilinear_tf(ctx):
    a = np.random.default_rng(42).normal(0, 1, (2, 9, 7, 5)).astype(np.float32)
    r = _lib.resize_bilinear_tf(ctx, ctx.to_device(a), 2, 9, 7, 5, 65, 48)
    return [host(ctx, r, (2, 65, 48, 5))]


def _u8_images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (hh, ww, 3)).astype(np.uint8) for hh, ww in ((75, 100), (100, 66), (65, 65), (1, 7))]


@case("msf-input-u8", "wsc_msf_input_u8")
def _msf_input(ctx):
    from tests import test_gpu_input as tin

    imgs = _u8_images()
    dev, offs, sizes = tin._pack_u8(ctx, imgs)
    outs = []
    for pair in (True, False):
        x = out(ctx, (len(imgs), 2 if pair else 1, 3, 65, 65))
        _lib.msf_input_u8(ctx, dev, sizes, offs, 65, (123.675, 116.28, 103.53), (58.395, 57.12, 57.375), x, pre_div255=False, pair=pair)
        outs.append(host(ctx, x, (len(imgs), 2 if pair else 1, 3, 65, 65)))
    return outs


@case("resize-u8", "wsc_resize_u8")
def _resize_u8(ctx):
    from tests import test_gpu_input as tin

    imgs = _u8_images()
    dev, offs, sizes = tin._pack_u8(ctx, imgs)
    outs = []
    for oh, ow in ((40, 56), (33, 33)):
        o = out(ctx, (len(imgs), oh, ow, 3), np.uint8)
        _lib.resize_u8(ctx, dev, sizes, offs, (oh, ow), o)
        outs.append(host(ctx, o, (len(imgs), oh, ow, 3), np.uint8))
    return outs


@case("pil-resize-u8", "wsc_pil_resize_u8")
def _pil_resize(ctx):
    from tests import test_gpu_irn_batch as tib

    outs = []
    for channels, order in ((3, 3), (1, 0), (1, 3)):
        outs += tib._run_resize(ctx, tib._resize_cases(channels), channels, order)
    return outs


@case("irn-train-batch", "wsc_irn_train_batch")
def _irn_train_batch(ctx):
    from tests import test_gpu_irn_batch as tib

    outs = []
    images, labels, params = tib._make_batch(tib._stage1_samples(), 32, 1)
    for norm, pre in ((tib.VOC_INT, False), (tib.VOC_FLOAT, True)):
        outs += list(tib._run_batch(ctx, images, labels, params, 32, norm, pre, 1))
    return outs


@case("seg-train-batch", "wsc_seg_train_batch")
def _seg_train_batch(ctx):
    from tests import test_gpu_seg_batch as tsb

    outs = []
    s, C = 9, 21
    tables = _lib.seg_cue_tables(*tsb._cue_lists(s, C))
    for lead in (tsb.GUARD, tsb.GUARD + 1):
        outs += list(tsb._train_batch(ctx, tsb._images(), tables, s, C, lead))
    return outs


@case("seg-gt-index-tf", "wsc_seg_gt_index_tf")
def _seg_gt_index(ctx):
    from tests import test_gpu_seg_batch as tsb

    gt3, gt1 = tsb._gts()
    return [tsb._gt_index(ctx, gt3, 3, tsb.COLOURS, 5, (33, 33)), tsb._gt_index(ctx, gt1, 1, None, 5, (33, 33))]


# ---- one mixed sequence: the production order of reuse -----------------------------------------------------------------------------
def _mixed_steps(ctx_of):
    """CRF build + inference, forward_edge, random walk, forward_cam: int tables, then half activations, in one arena.  ctx_of(i): the
    context step i runs on.  Everything is uploaded and allocated (and the nets are packed) before the first of the four calls;
    between them the host waits for nothing but what wsc_crf_create waits for itself, and reads back after the last."""
    from tests import helpers

    rng = np.random.default_rng(77)
    H, W, M = 47, 61, 5
    cases = [helpers.synth_crf_case(rng, H, W, M) for _ in range(2)]
    c0, c1, c2, c3 = (ctx_of(i) for i in range(4))
    rgb_dev, u_dev = c0.to_device(np.stack([c[0] for c in cases])), c0.to_device(np.stack([c[1] for c in cases]))
    q_dev, a_dev = out(c0, (2, M, H * W)), out(c0, (2, H * W), np.int32)
    with irn_model(c1, "resnet50", _lib.PREC_F16X3) as m, cam_net(c3, "resnet50", _lib.PREC_F16X3) as cnet:
        net = m._net
        (He, We), _ = net.edge_size(64)
        hc = cnet.cam_size(64)
        x_dev = c1.to_device(_edge_input(2, 64))
        e_dev, d_dev = out(c1, (1, He, We)), out(c1, (1, 2, He, We))
        rx_dev, re_dev = _rw_upload(c2)
        n_rw = sum(int(np.prod(s)) for s in RW_SHAPES)
        rw_dev = out(c2, (n_rw,))
        xc_dev, cam_dev = c3.to_device(_cam_input(2, 64, 64)), out(c3, (2, 20, hc, hc))
        crf = _lib.Crf(c0, rgb_dev, 2, H, W, CRF_CFG[0], CRF_CFG[2], CRF_CFG[3])
        try:
            crf.inference(u_dev, M, CRF_CFG[1], CRF_CFG[4], CRF_CFG[5], q_dev, a_dev)
            net.forward_edge(x_dev, 1, 64, He, We, e_dev, d_dev)
            _rw_run(c2, rx_dev, re_dev, rw_dev)
            cnet.forward_cam(xc_dev, 2, 64, cam_dev, None)
            return [host(c0, q_dev, (2, M, H * W)), host(c0, a_dev, (2, H * W), np.int32), host(c1, e_dev, (1, He, We)),
                    host(c1, d_dev, (1, 2, He, We)), host(c2, rw_dev, (n_rw,)), host(c3, cam_dev, (2, 20, hc, hc))]
        finally:
            crf.close()


def test_mixed_sequence_on_one_context_equals_fresh_contexts():
    """The four calls back to back on ONE fresh context under fill 0xFF -- every call finds the arena and the cached blocks as the
    call before left them, or 0xFF -- against each call on a fresh context of its own without a fill."""
    one = _lib.Context(0)
    try:
        with guarded_allocations(one, 0xFF), one.scratch_fill(0xFF):
            got = [np.array(a, copy=True) for a in _mixed_steps(lambda i: one)]
    finally:
        one.close()
    own = [_lib.Context(0) for _ in range(4)]
    try:
        with contextlib.ExitStack() as stack:
            for c in own:
                stack.enter_context(guarded_allocations(c, 0xA5))
            want = [np.array(a, copy=True) for a in _mixed_steps(lambda i: own[i])]
    finally:
        for c in own:
            c.close()
    assert len(got) == len(want) == 6
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (k, int((bits(a) != bits(b)).sum()))


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(_RUNS))
def test_result_does_not_depend_on_scratch(ctx, cid):
    sweep(ctx, cid)


def test_scratch_fill_argument_and_restore(ctx):
    """0 .. 255 and -1 are the values; anything else is WSC_ERR_INVALID and changes nothing, on or off; the context manager turns
    the fill off again when the block raises (the hook's state: wsc_ctx_scratch_fill_value)."""
    assert ctx.scratch_fill_value() == -1
    for bad in (-2, 256, 1 << 20):
        assert ctx._lib.wsc_ctx_scratch_fill(ctx.h, bad) == _lib.WSC_ERR_INVALID
        assert ctx.scratch_fill_value() == -1
    assert ctx._lib.wsc_ctx_scratch_fill(None, 0) == _lib.WSC_ERR_INVALID
    with pytest.raises(RuntimeError):
        with ctx.scratch_fill(0xFF):
            assert ctx.scratch_fill_value() == 0xFF
            assert ctx._lib.wsc_ctx_scratch_fill(ctx.h, 256) == _lib.WSC_ERR_INVALID
            assert ctx.scratch_fill_value() == 0xFF  # (a refused value leaves the hook as it was)
            raise RuntimeError("inside")
    assert ctx.scratch_fill_value() == -1
