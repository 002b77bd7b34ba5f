"""TEST INFRASTRUCTURE ONLY (oracle) -- the backward pass of the IRNet heads, restated by hand in float64.

    head_table(arch)   the heads, concat buffers and final convs of an EdgeDisplacement net, from oracle/irn_ref.py's *_HEADS
    host_tape(x, sd, arch)  a self-consistent float64 forward pass with torch on the CPU -> (tape, edge_out, dp_out); the tape
                       is a dict under the names of wsc_net_edge_tape_plan: "x<k>" [N][H][W][C] stage taps, "<head>.z" the conv
                       outputs, "<head>.stats" [N][1][1][2 G] {mean, rstd} pairs, "cat<i>" [N][Hc][Wc][Ctot] concat buffers
                       (padding channels included, zeros)
    head_grads(tape, sd, arch, d_edge, d_dp)  the MANUAL chain rule at that tape -> {state-dict name: gradient in torch's
                       shape}: ReLU masks from the taped concat values (> 0), xh from the taped z with float64 statistics (the
                       taped float pair is not read), upsample adjoint from the forward's weights, stage taps detached
    replay(tape, sd, arch)  every z / stats / cat entry recomputed in float64 FROM THE ENTRIES IT READ (the per-op check of a
                       device tape)
    up_relu_grad / group_norm_grad  the float64 forms of the two per-op kernels

tests/test_irn_grad_oracle.py holds head_grads against torch.double autograd and measures the two constants below.

R32_GN         over GN_CASES (without the constant-group case, where float32 autograd itself is 30 x worse on dgamma), the worst
               max|g32 - g64| / max|g64| of torch float32 autograd of F.group_norm against float64 on identical float32
               operands, per output (dz, dgamma, dbeta).
R32_IRN_CHAIN  the same ratio per parameter for head_grads run in float32 against float64 on one float32 tape (resnet50,
               S = 64, N = 2, d_edge, d_dp = 1e-3 N(0, 1)); the worst parameter is the figure.
The GPU bounds are multiples of these (tests/test_gpu_irn_grad.py); the oracle test holds re-measured figures to 1.5 x."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn_ref, irn_ref

R32_GN = {"dz": 1.21e-7, "dgamma": 2.63e-7, "dbeta": 2.70e-7}  # worst cases: (3, 17, 17, 64, 8) / (1, 33, 32, 32, 4) twice
R32_IRN_CHAIN = 1.13e-6  # at fc_dp1.1.weight

# (N, H, W, C, G); the last one is run with group 1 of sample 0 constant
GN_CASES = [(1, 1, 1, 32, 4), (2, 5, 3, 32, 4), (1, 9, 9, 256, 16), (3, 17, 17, 64, 8), (1, 33, 32, 32, 4), (2, 4, 4, 128, 16)]
GN_CONSTANT_CASE = (2, 6, 5, 32, 4)
EPS = 1e-5


def head_table(arch):
    """-> dict(heads=[dict(name, src=('x', k) | ('cat', i), stride, cout, groups, up, dst, coff)] in execution order,
    cats=[(channels, stage whose resolution it has)], edge_final, edge_in, dp_final, stage_channels)"""
    spec = {"resnet50": irn_ref.RESNET50_HEADS, "vgg16": irn_ref.VGG16_HEADS, "m7": irn_ref.M7_HEADS}[arch]
    heads = []
    for i, (name, src, stride, cout, groups, up) in enumerate(spec["edge"]):
        heads.append(dict(name=name, src=("x", src), stride=stride, cout=cout, groups=groups, up=up, dst=0, coff=32 * i))
    if arch == "m7":
        place = {"fc_dp1": (2, 0), "fc_dp2": (2, 64), "fc_dp3": (1, 0)}
        chained = [("fc_dp4", 1, 2, 2, 192), ("fc_dp5", 2, 1, 3, 0)]
        cats = [(128, 1), (256, 3), (448, 2), (256, 2)]
        finals = ("fc_edge4", 96, "fc_dp5.3")
    else:
        place = {"fc_dp1": (2, 0), "fc_dp2": (2, 64), "fc_dp3": (1, 0), "fc_dp4": (1, 256), "fc_dp5": (1, 512)}
        chained = [("fc_dp6", 1, 2, 2, 192), ("fc_dp7", 2, 1, 3, 0)]
        cats = [(192, 2), (768, 3), (448, 2), (256, 2)]
        finals = ("fc_edge6", 160, "fc_dp7.3")
    for name, src, stride, cout, groups, up in spec["dp"]:
        heads.append(dict(name=name, src=("x", src), stride=stride, cout=cout, groups=groups, up=up, dst=place[name][0], coff=place[name][1]))
    for name, src_cat, up, dst, coff in chained:
        heads.append(dict(name=name, src=("cat", src_cat), stride=1, cout=256, groups=16, up=up, dst=dst, coff=coff))
    return dict(heads=heads, cats=cats, edge_final=finals[0], edge_in=finals[1], dp_final=finals[2], stage_channels=spec["stage_channels"])


def param_names(arch):
    """the state-dict names of trainable_parameters(): (edge_layers, dp_layers)"""
    t = head_table(arch)
    edge, dp = [], []
    for h in t["heads"]:
        (edge if h["dst"] == 0 else dp).extend([h["name"] + ".0.weight", h["name"] + ".1.weight", h["name"] + ".1.bias"])
    return edge + [t["edge_final"] + ".weight", t["edge_final"] + ".bias"], dp + [t["dp_final"] + ".weight"]


def stages(x, sd, arch):
    if arch == "resnet50":
        return irn_ref.resnet50_stages(x, sd)
    if arch == "vgg16":
        return irn_ref.vgg16_stages(x, sd)
    out = []
    for stage in irn_ref.M7_STAGES:
        x = cnn_ref.plain_features(x, sd, "m7", stage)
        out.append(x)
    return out


def axis_matrix(n_dst, n_src, up, dtype=np.float64):
    """R [n_dst][n_src]: row d holds the two bilinear weights of destination d as the forward kernel forms them in float32
    (src = (d + 0.5) / up - 0.5 clamped at 0; the second tap stays on the last pixel); up = 1: the identity rows"""
    R = np.zeros((n_dst, n_src), dtype)
    for d in range(n_dst):
        if up == 1:
            R[d, d] = 1
            continue
        s = np.float32(np.float32(d + 0.5) * np.float32(1.0 / up) - np.float32(0.5))
        s = max(s, np.float32(0))
        i0 = int(s)
        i1 = i0 + (1 if i0 < n_src - 1 else 0)
        l = np.float32(s - np.float32(i0))
        R[d, i0] += np.float32(1) - l
        R[d, i1] += l
    return R


def up_relu_grad(dcat, cat, H, W, C, up, coff, dtype=np.float64):
    """dy [N][H][W][C], sum|terms| per element and its count of non-zero terms, of the adjoint of upsample-crop-ReLU-slice"""
    N, Hd, Wd, _ = dcat.shape
    g = np.where(cat[..., coff:coff + C] > 0, dcat[..., coff:coff + C], 0).astype(dtype)
    Ry, Rx = axis_matrix(Hd, H, up, dtype), axis_matrix(Wd, W, up, dtype)
    dy = np.einsum("hy,wx,nhwc->nyxc", Ry, Rx, g)
    mag = np.einsum("hy,wx,nhwc->nyxc", Ry, Rx, np.abs(g))
    terms = np.einsum("hy,wx,nhwc->nyxc", (Ry > 0).astype(np.float64), (Rx > 0).astype(np.float64), (g != 0).astype(np.float64))
    return dy, mag, terms


def group_stats(z, G):
    """float64 (mean, rstd) [N][G] of z [N][H][W][C]"""
    N, H, W, C = z.shape
    zz = z.astype(np.float64).reshape(N, H * W, G, C // G)
    mean = zz.mean(axis=(1, 3))
    var = (zz * zz).mean(axis=(1, 3)) - mean * mean
    return mean, 1.0 / np.sqrt(np.maximum(var, 0) + EPS)


def group_norm_grad(z, dy, gamma, G, dtype=np.float64):
    """(dz, dgamma, dbeta) of GroupNorm(G, C) at z [N][H][W][C], statistics in float64 from z"""
    N, H, W, C = z.shape
    Cg = C // G
    mean, rstd = group_stats(z, G)
    mean, rstd = np.repeat(mean, Cg, axis=1).astype(dtype), np.repeat(rstd, Cg, axis=1).astype(dtype)
    z, dy, gamma = z.astype(dtype), dy.astype(dtype), gamma.astype(dtype)
    xh = (z - mean[:, None, None, :]) * rstd[:, None, None, :]
    A, B = dy.sum(axis=(1, 2)), (dy * xh).sum(axis=(1, 2))  # [N][C]
    m = dtype(Cg * H * W)
    m1 = np.repeat((gamma * A).reshape(N, G, Cg).sum(axis=2) / m, Cg, axis=1)
    m2 = np.repeat((gamma * B).reshape(N, G, Cg).sum(axis=2) / m, Cg, axis=1)
    dz = rstd[:, None, None, :] * (gamma * dy - m1[:, None, None, :] - xh * m2[:, None, None, :])
    return dz, B.sum(axis=0), A.sum(axis=0)


def _nhwc(t):
    return np.ascontiguousarray(t.detach().permute(0, 2, 3, 1).numpy())


def _apply_head(z, stats_or_none, gamma, beta, G, up, Hd, Wd):
    """GroupNorm (float64 statistics from z) -> upsample -> crop -> ReLU of z [N][H][W][C], float64"""
    N, H, W, C = z.shape
    mean, rstd = group_stats(z, G)
    Cg = C // G
    y = (z.astype(np.float64) - np.repeat(mean, Cg, 1)[:, None, None, :]) * np.repeat(rstd, Cg, 1)[:, None, None, :] * gamma + beta
    Ry, Rx = axis_matrix(Hd, H, up), axis_matrix(Wd, W, up)
    return np.maximum(np.einsum("hy,wx,nyxc->nhwc", Ry, Rx, y), 0)


def _walk(xs, sd, arch, table, conv_in):
    """the forward pass of the heads in float64 numpy; conv_in(kind, index, computed) picks what a conv reads: the tensor just
    computed (host_tape) or the tape's own entry (replay) -> the tape dict"""
    w = {k: v.detach().double().numpy() if hasattr(v, "detach") else np.asarray(v, np.float64) for k, v in sd.items()
         if k.startswith("fc_")}
    tape = {}
    N = xs[0].shape[0]
    res = {k + 1: xs[k].shape[1:3] for k in range(len(xs))}
    cats = [np.zeros((N,) + tuple(res[stage]) + (ch,)) for ch, stage in table["cats"]]
    for h in table["heads"]:
        kind, k = h["src"]
        x = conv_in(kind, k, xs[k - 1] if kind == "x" else cats[k])
        x = x[:, ::h["stride"], ::h["stride"], :].astype(np.float64)
        z = x @ w[h["name"] + ".0.weight"][:, :, 0, 0].T
        tape[h["name"] + ".z"] = z
        z = conv_in("z", h["name"], z)
        mean, rstd = group_stats(z, h["groups"])
        tape[h["name"] + ".stats"] = np.stack([mean, rstd], axis=2).reshape(N, 1, 1, 2 * h["groups"])
        Hd, Wd = cats[h["dst"]].shape[1:3]
        cats[h["dst"]][..., h["coff"]:h["coff"] + h["cout"]] = _apply_head(z, None, w[h["name"] + ".1.weight"], w[h["name"] + ".1.bias"],
                                                                           h["groups"], h["up"], Hd, Wd)
    for i, c in enumerate(cats):
        tape["cat%d" % i] = c
    c0, cl = conv_in("cat", 0, cats[0]).astype(np.float64), conv_in("cat", len(cats) - 1, cats[-1]).astype(np.float64)
    ein = table["edge_in"]
    edge = c0[..., :ein] @ w[table["edge_final"] + ".weight"][0, :, 0, 0] + w[table["edge_final"] + ".bias"][0]
    dp = np.moveaxis(cl @ w[table["dp_final"] + ".weight"][:, :, 0, 0].T, 3, 1)
    return tape, edge, dp


def host_tape(x, sd, arch):
    """x float (N, 3, S, S), sd a torch state dict -> (tape, edge_out [N][He][We], dp_out [N][2][Hd][Wd]), all float64; the
    backbone runs in torch.double, so the tape is self-consistent: every entry is the float64 op on the entries before it"""
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        xs = [_nhwc(t) for t in stages(torch.as_tensor(x).double(), sd64, arch)]
    table = head_table(arch)
    tape, edge, dp = _walk(xs, sd, arch, table, lambda kind, k, computed: computed)
    for h in table["heads"]:
        if h["src"][0] == "x":
            tape["x%d" % h["src"][1]] = xs[h["src"][1] - 1]
    return tape, edge, dp


def replay(tape, sd, arch):
    """a (device) tape -> the dict of its z / stats / cat entries recomputed in float64, each from the tape's own entries it
    read: z from the tap or concat entry, stats and the concat slices from the z entries"""
    table = head_table(arch)
    xs = [tape["x%d" % (k + 1)] for k in range(len(table["stage_channels"]))]  # (every stage of the three nets has a head)

    def pick(kind, k, computed):
        if kind == "x":
            return tape["x%d" % k]
        if kind == "cat":
            return tape["cat%d" % k]
        return tape[k + ".z"]

    return _walk(xs, sd, arch, table, pick)[0]


def head_grads(tape, sd, arch, d_edge, d_dp, dtype=np.float64):
    """the manual backward pass at `tape` -> {state-dict name: gradient}, computed in `dtype` (float64: the oracle; float32: the
    measurement behind R32_IRN_CHAIN).  The GroupNorm statistics are float64 from the taped z in both."""
    table = head_table(arch)
    w = {k: np.asarray(v.detach().numpy() if hasattr(v, "detach") else v).astype(dtype) for k, v in sd.items() if k.startswith("fc_")}
    t = {k: np.asarray(v) for k, v in tape.items()}
    d_edge, d_dp = np.asarray(d_edge).astype(dtype), np.asarray(d_dp).astype(dtype)
    nc = len(table["cats"])
    out, dcat = {}, [None] * nc
    ein, ef, df = table["edge_in"], table["edge_final"], table["dp_final"]
    c0 = t["cat0"].astype(dtype)
    out[ef + ".weight"] = np.einsum("nhwc,nhw->c", c0[..., :ein], d_edge).reshape(1, ein, 1, 1)
    out[ef + ".bias"] = d_edge.sum().reshape(1)
    dcat[0] = np.zeros(c0.shape, dtype)
    dcat[0][..., :ein] = d_edge[..., None] * w[ef + ".weight"][0, :, 0, 0]
    cl = t["cat%d" % (nc - 1)].astype(dtype)
    out[df + ".weight"] = np.einsum("nhwc,nkhw->kc", cl, d_dp)[:, :, None, None]
    dcat[nc - 1] = np.einsum("nkhw,kc->nhwc", d_dp, w[df + ".weight"][:, :, 0, 0])
    for h in reversed(table["heads"]):
        name, C = h["name"], h["cout"]
        z = t[name + ".z"]
        H, W = z.shape[1:3]
        dy = up_relu_grad(dcat[h["dst"]], t["cat%d" % h["dst"]], H, W, C, h["up"], h["coff"], dtype)[0]
        dz, dgamma, dbeta = group_norm_grad(z, dy, w[name + ".1.weight"], h["groups"], dtype)
        kind, k = h["src"]
        x = (t["x%d" % k] if kind == "x" else t["cat%d" % k]).astype(dtype)[:, ::h["stride"], ::h["stride"], :]
        out[name + ".0.weight"] = np.einsum("nhwi,nhwo->oi", x, dz)[:, :, None, None]
        out[name + ".1.weight"], out[name + ".1.bias"] = dgamma, dbeta
        if kind == "cat":  # (stage taps are detached)
            dcat[k] = np.einsum("nhwo,oi->nhwi", dz, w[name + ".0.weight"][:, :, 0, 0])
    return out


def worst_ratio(got, want):
    """-> (worst max|got - want| / max|want| over the parameters, its name)"""
    worst = (0.0, "")
    for name, g in want.items():
        top = np.abs(g).max()
        r = float(np.abs(np.asarray(got[name], np.float64) - g).max() / top) if top > 0 else 0.0
        worst = max(worst, (r, name))
    return worst


def gn_case(case, seed, constant=False):
    """-> z, dy [N][H][W][C] float32, gamma [C] float32"""
    N, H, W, C, G = case
    rng = np.random.default_rng(seed)
    z = rng.normal(0.3, 1.5, (N, H, W, C)).astype(np.float32)
    if constant:
        Cg = C // G
        z[0, :, :, Cg:2 * Cg] = np.float32(0.75)
    dy = rng.normal(0, 1, (N, H, W, C)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    return z, dy, gamma


def torch_gn_grads(z, dy, gamma, G, dtype):
    """torch autograd of F.group_norm on NHWC operands -> (dz [N][H][W][C], dgamma, dbeta)"""
    zt = torch.from_numpy(z).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gt = torch.from_numpy(gamma).to(dtype).requires_grad_(True)
    bt = torch.zeros(len(gamma), dtype=dtype, requires_grad=True)
    y = F.group_norm(zt, G, gt, bt, eps=EPS)
    y.backward(torch.from_numpy(dy).to(dtype).permute(0, 3, 1, 2))
    return zt.grad.permute(0, 2, 3, 1).numpy(), gt.grad.numpy(), bt.grad.numpy()
