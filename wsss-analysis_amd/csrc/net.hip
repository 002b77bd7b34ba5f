// net.hip -- host side of the CAM networks: state_dict -> packed device weights, and the
// per-batch launch sequence.
//
// Reference being replaced:
//   resnet50_cam : 03b_irn/net/resnet50.py:17-108 assembled by resnet50_cam.py:12-20 with
//                  strides=(2,2,2,1); CAM.forward resnet50_cam.py:55-70
//   vgg16_cam    : net/vgg16.py:44 cfg + common_cnn.py:128-141 make_layers
//                  (conv(bias) -> ReLU -> BatchNorm(eps=1e-3)); vgg16_cam.py:24-50
//   m7_cam       : net/m7.py:41 cfg; m7_cam.py:22-47 (Grad-CAM weights as the 1x1 head)
//   construction/load: 03b_irn/step/make_cam.py:96-100
//   deeplab_lfov / deeplab_aspp : the DeepLab-VGG16 of 03a_sec-dsrg, SEC.py:117-128 / DSRG.py:169-186 (build_block, build_fc):
//                  forward pass at drop_prob = 0, weights under the reference's layer names in TF's HWIO order
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

namespace {

struct HostTensor {
    const float *data;
    int ndim;
    int64_t shape[4];
    int64_t numel() const {
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= shape[i];
        return n;
    }
};
typedef std::unordered_map<std::string, HostTensor> Dict;

struct ConvW {
    void *w = nullptr; // packed weights: 16-bit, fp32 in WSC_PREC_F32 (make_conv)
    float *s1 = nullptr, *b1 = nullptr, *s2 = nullptr, *b2 = nullptr;
    int Cin = 0, Cout = 0, CoutPad = 0, kh = 1, kw = 1, stride = 1, pad = 0, relu = 0;
    int dil = 1; // dilation (tf.nn.atrous_conv2d's rate); make_conv leaves 1, the DeepLab builder sets it
    ConvForm form = CONV_FORM_GENERIC;
    int bn = -1; // plain stacks: the layer's BatchNorm in wsc_net::bns (s2 / b2 is its inference form), -1 without one
};
// the BatchNorm behind a conv -> ReLU of a plain stack as the training pass needs it (wsc_net_forward_cls_train): the affine
// parameters themselves, not folded with the running statistics
struct PlainBn {
    std::string name;                        // the state-dict prefix: `<name>.{weight,bias,running_mean,running_var}`
    float *gamma = nullptr, *beta = nullptr; // device, [C]
    int C = 0;
    float eps = 1e-3f;
    double eps_fold = 1e-3; // the eps fold_bn took for s2 / b2 (the double constant, or the state dict's float): wsc_net_cls_load_params
};

// one Conv2d(1x1, bias=False) -> GroupNorm -> [Upsample] -> ReLU head of the IRNet branches
struct IrnHead {
    std::string name; // the state-dict prefix: `<name>.0.weight`, `<name>.1.{weight,bias}`
    ConvW conv;
    int groups = 1, up = 1;
    float *gamma = nullptr, *beta = nullptr; // device, [Cout]
    int src = 0;                             // stage k (1-based) when > 0, concat buffer -src - 1 when < 0
    int dst = 0, coff = 0;                   // destination concat buffer and channel offset inside it
};
// a concat buffer: NHWC with `channels` channels at the resolution of stage `stage` divided by `stride`
struct IrnCat {
    int channels, stage, stride;
};

enum OpType { OP_CONV = 0, OP_POOL = 1, OP_GATHER = 2 };
// one row of `pool_spec`
struct PoolSpec {
    int k, stride, same;
    PoolRule rule() const { return same ? POOL_TF_SAME : POOL_TF_VALID; }
};
// one fc6 (3x3 atrous) -> fc7 (1x1) -> fc8 (1x1, no ReLU, fp32 logits) branch of the DeepLab head
struct SegBranch {
    ConvW fc6, fc7, fc8;
};
// (made by add_conv_op / add_pool_op / add_gather_op only)
struct Op {
    int type = OP_CONV;
    int conv = -1;                  // index into convs (OP_CONV)
    int in = -1, out = 0, res = -1; // activation buffer ids; res = -1 if none; in = -1 means the NHWC4 input
    PoolRule rule = POOL_TORCH;     // OP_POOL: how the window meets the border (pool_geom)
    int pk = 0, ps = 0, pp = 0;     // OP_POOL: window / stride / torch pad (POOL_TORCH only); OP_GATHER, OP_CONV with in2: ps = pixel stride
    bool avg = false;               // OP_POOL: the average instead of the maximum
    int pitch = 0;                  // channels per output row when the op writes a channel range of a wider (concatenated) tensor, else 0
    int coff = 0;                   // first channel of that range
    int drop_site = -1;             // OP_CONV of a plain stack: the dropout site behind it (a 'D' entry, in table order), -1 without one
    int in2 = -1;                   // OP_CONV, 1x1: buffer whose pixels (ho * ps, wo * ps) supply the LAST input channels (ConvLaunch::x2), or -1
    std::string label;              // the state-dict layers the op implements (wsc_net_trace_plan): a conv's weight key without ".weight",
                                    // "<block>.conv3+downsample" for the stage-entry GEMM, "<block>.gather", "pool:<ordinal>"
};

} // namespace

struct wsc_net {
    wsc_ctx *ctx = nullptr;
    int arch = 0, C = 0, F = 0;
    wsc_precision prec = WSC_PREC_BF16;
    std::vector<ConvW> convs;
    std::vector<Op> ops;
    int final_buf = 0;
    ConvW head;
    bool head_is_cls = false; // vgg16 without `gradcam_weights`: the head's rows are the classifier's Linear (wsc_net_cls_load_params)
    float *cls_w = nullptr, *cls_b = nullptr; // classifier branch (vgg16 / m7), fp32 [Ccls][F]
    int Ccls = 0;
    int cls_max = 0; // 1: global max pooling (m7), 0: global average (vgg16)
    bool cls_pool_set = false; // m7 with a `pool_spec`: its third row, the classifier branch's layer3_p2 pool
    PoolSpec cls_pool = {2, 2, 0};
    // IRNet EdgeDisplacement (arch >= WSC_ARCH_RESNET50_IRN): backbone stage taps + the two head branches
    std::vector<int> taps;       // op index whose output is stage k+1 (x1..x5)
    std::vector<IrnHead> heads;  // every Conv-GroupNorm-[Upsample]-ReLU head in execution order
    std::vector<IrnCat> cats;    // concat buffers; cats[0] feeds the final edge conv, cats.back() the final dp conv
    ConvW edge6, dp7b;           // final edge conv (bias) / final displacement conv
    std::string edge_final, dp_final; // their state-dict names without ".weight"
    int edge_in = 0;             // input channels of the final edge conv before the padding to cats[0].channels
    float mean_shift[2] = {0.f, 0.f};
    std::vector<SegBranch> seg;  // WSC_ARCH_DEEPLAB_*: one branch (LFOV, SEC) or four (ASPP, DSRG); fc8 = their sum
    std::vector<PlainBn> bns;    // the BatchNorm layers of a plain stack in stack order (ConvW::bn)
    std::vector<void *> allocs;
};

namespace {

// the precision argument of the C ABI
int decode_precision(int precision, wsc_precision *prec) {
    WSC_CHECK(precision == WSC_PREC_BF16 || precision == WSC_PREC_BF16X3 || precision == WSC_PREC_F16 || precision == WSC_PREC_F16X3 ||
                  precision == WSC_PREC_F32,
              WSC_ERR_INVALID, "unknown precision %d", precision);
    *prec = (wsc_precision)precision;
    return WSC_OK;
}

int upload(wsc_net *net, const void *host, size_t bytes, void **out) {
    void *d = nullptr;
    WSC_HIP(hipMalloc(&d, bytes));
    net->allocs.push_back(d);
    WSC_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    *out = d;
    return WSC_OK;
}

int get(const Dict &d, const std::string &k, int ndim, const HostTensor **out) {
    auto it = d.find(k);
    WSC_CHECK(it != d.end(), WSC_ERR_MISSING_KEY, "state_dict: missing key '%s'", k.c_str());
    WSC_CHECK(it->second.ndim == ndim, WSC_ERR_SHAPE, "state_dict: '%s' has ndim %d, expected %d", k.c_str(),
              it->second.ndim, ndim);
    WSC_CHECK(it->second.data != nullptr, WSC_ERR_INVALID, "state_dict: '%s' has a null data pointer", k.c_str());
    *out = &it->second;
    return WSC_OK;
}
bool has(const Dict &d, const std::string &k) { return d.find(k) != d.end(); }

// the wsc_tensor_desc list of the C ABI as a dictionary (the data stays the caller's)
int descs_to_dict(const wsc_tensor_desc *weights, int n_weights, Dict *d) {
    for (int i = 0; i < n_weights; ++i) {
        WSC_CHECK(weights[i].name != nullptr, WSC_ERR_INVALID, "weights[%d].name is null", i);
        WSC_CHECK(weights[i].ndim >= 0 && weights[i].ndim <= 4, WSC_ERR_SHAPE, "'%s': ndim %d unsupported",
                  weights[i].name, weights[i].ndim);
        HostTensor t;
        t.data = weights[i].data;
        t.ndim = weights[i].ndim;
        for (int k = 0; k < 4; ++k) t.shape[k] = k < t.ndim ? weights[i].shape[k] : 1;
        if (t.ndim == 0) { t.ndim = 1; t.shape[0] = 1; }
        (*d)[weights[i].name] = t;
    }
    return WSC_OK;
}

// Fold inference batch-norm y = (x - mean) / sqrt(var + eps) * gamma + beta into scale/shift.
int fold_bn(const Dict &d, const std::string &bn, int C, double eps_default, std::vector<float> &s,
            std::vector<float> &b) {
    const HostTensor *g, *be, *mu, *var;
    WSC_TRY(get(d, bn + ".weight", 1, &g));
    WSC_TRY(get(d, bn + ".bias", 1, &be));
    WSC_TRY(get(d, bn + ".running_mean", 1, &mu));
    WSC_TRY(get(d, bn + ".running_var", 1, &var));
    WSC_CHECK(g->shape[0] == C && be->shape[0] == C && mu->shape[0] == C && var->shape[0] == C, WSC_ERR_SHAPE,
              "state_dict: batch-norm '%s' is not %d channels", bn.c_str(), C);
    double eps = eps_default;
    auto it = d.find(bn + ".eps");
    if (it != d.end() && it->second.data) eps = it->second.data[0];
    s.resize(C);
    b.resize(C);
    for (int c = 0; c < C; ++c) {
        const double sc = (double)g->data[c] / std::sqrt((double)var->data[c] + eps);
        s[c] = (float)sc;
        b[c] = (float)((double)be->data[c] - (double)mu->data[c] * sc);
    }
    return WSC_OK;
}

// Pack OIHW fp32 weights to [CoutPad][Kw] 16-bit in the kernel's K order (conv_k_layout, common.h); WSC_PREC_F32: the fp32
// values themselves in that order -- no rounding, no power-of-two packing.
int make_conv(wsc_net *net, const HostTensor *w, int stride, int pad, int relu, ConvForm form,
              const std::vector<float> &s1, const std::vector<float> &b1, const std::vector<float> *s2,
              const std::vector<float> *b2, ConvW *out) {
    const int Cout = (int)w->shape[0], Cin = (int)w->shape[1], kh = (int)w->shape[2], kw = (int)w->shape[3];
    ConvW c;
    c.Cout = Cout;
    c.CoutPad = conv_cout_pad(Cout);
    c.kh = kh; c.kw = kw; c.stride = stride; c.pad = pad; c.relu = relu; c.form = form;
    if (form == CONV_FORM_GENERIC) {
        WSC_CHECK(Cin % 64 == 0, WSC_ERR_SHAPE, "conv with Cin=%d is not supported (need a multiple of 64)", Cin);
        c.Cin = Cin;
    } else if (form == CONV_FORM_STEM_ROWS) {
        WSC_CHECK(Cin <= 4 && kw <= 7 && conv_split(net->prec) == 2, WSC_ERR_SHAPE, "padded-stem conv needs Cin <= 4, kw <= 7, f16x3");
        c.Cin = 4;
    } else {
        WSC_CHECK(Cin <= 4, WSC_ERR_SHAPE, "small-Cin conv needs Cin <= 4, got %d", Cin);
        WSC_CHECK(kw <= (form == CONV_FORM_SMALL2 ? 4 : 8), WSC_ERR_SHAPE, "small-Cin conv: kw=%d too wide", kw);
        c.Cin = 4;
    }
    const ConvKLayout lay = conv_k_layout(kh, kw, c.Cin, form, net->prec);
    const int Kw = lay.Kw;
    const bool f32 = net->prec == WSC_PREC_F32;
    const int fmt = conv_fmt(net->prec), split = conv_split(net->prec);
    std::vector<char> wp((size_t)c.CoutPad * Kw * conv_elem_bytes(net->prec), 0); // (zero bits = 0 in every format)
    // IEEE-half modes (f16, f16x3): every output channel's weights are stored times a power of two that puts the channel's
    // largest |w| into [2^12, 2^13), and the epilogue scale s1 takes the inverse -- exact in fp32, the accumulators are fp32.
    // Half has 5 exponent bits: a checkpoint's late-layer weights (|w| ~ 1e-4 ... 1e-3, below half's smallest normal
    // 6.1e-5 for many of them) would lose their `hi` bits and all of `lo` (the split's lo = half(w - hi) is ~2^-11 |w|);
    // scaled, every weight within 2^-15 of its channel's maximum keeps the full 22-bit hi + lo pair and smaller ones an
    // absolute error of 2^-25 against a maximum of >= 2^12 (bfloat16 has fp32's exponent range).
    std::vector<float> s1v(s1);
    std::vector<float> wscale(Cout, 1.f);
    if (fmt == 1) {
        const size_t per = (size_t)Cin * kh * kw;
        // the door of the range guard for what the host packs: a half cannot hold NaN / inf (the saturating conversion would
        // store +-65504 for an inf and raise nothing, std::max below passes over a NaN), so an IEEE-half layer takes none
        for (size_t i = 0; i < per * Cout; ++i)
            WSC_CHECK(std::isfinite(w->data[i]), WSC_ERR_RANGE,
                      "a weight of an IEEE-half layer is not finite (%g, output channel %d of %d): WSC_PREC_F32 computes with it, as the reference does",
                      (double)w->data[i], (int)(i / per), Cout);
        for (const std::vector<float> *v : {&s1, &b1, s2, b2})
            for (int co = 0; v && co < Cout; ++co)
                WSC_CHECK(std::isfinite((*v)[co]), WSC_ERR_RANGE,
                          "a scale / shift of an IEEE-half layer is not finite (%g, output channel %d of %d): WSC_PREC_F32 computes with it, as the reference does",
                          (double)(*v)[co], co, Cout);
        for (int co = 0; co < Cout; ++co) {
            float mx = 0.f;
            for (size_t i = 0; i < per; ++i) mx = std::max(mx, std::fabs(w->data[(size_t)co * per + i]));
            // (bounded shift: a dead channel in fp32's denormal range -- weight decay leaves |w| ~ 1e-40 -- would otherwise
            // ask for 2^(13 - e) = inf, every weight * inf = inf, lo = inf - inf = NaN; with the bound such a channel keeps
            // its tiny values as half subnormals / zeros like before the packing)
            const int sh = conv_half_shift(mx); // (common.h: the device repack of repack.hip takes the same shift)
            wscale[co] = conv_pow2(sh);
            s1v[co] = s1[co] * conv_pow2(-sh);
        }
    }
    for (int co = 0; co < Cout; ++co) {
        bf16_t *row = f32 ? nullptr : (bf16_t *)wp.data() + (size_t)co * Kw;
        float *row_f32 = f32 ? (float *)wp.data() + (size_t)co * Kw : nullptr;
        const float wsc = wscale[co];
        auto put = [&](int k, float v) {
            if (f32) { // the weight itself
                row_f32[k] = v;
                return;
            }
            v *= wsc;
            const bf16_t h = f32_to_h16(v, fmt);
            row[k] = h;
            if (split) row[lay.lo_at + k] = f32_to_h16(v - h16_to_f32(h, fmt), fmt);
        };
        for (int ci = 0; ci < Cin; ++ci)
            for (int r = 0; r < kh; ++r)
                for (int s = 0; s < kw; ++s) put(lay.index(ci, r, s), w->data[(((size_t)co * Cin + ci) * kh + r) * kw + s]);
    }
    WSC_TRY(upload(net, wp.data(), wp.size(), &c.w));
    auto up_vec = [&](const std::vector<float> &v, float **dst) -> int {
        std::vector<float> p(c.CoutPad, 0.f);
        for (int i = 0; i < Cout; ++i) p[i] = v[i];
        return upload(net, p.data(), p.size() * sizeof(float), (void **)dst);
    };
    WSC_TRY(up_vec(s1v, &c.s1));
    WSC_TRY(up_vec(b1, &c.b1));
    if (s2) {
        WSC_TRY(up_vec(*s2, &c.s2));
        WSC_TRY(up_vec(*b2, &c.b2));
    }
    *out = c;
    return WSC_OK;
}

// The weight- and precision-derived fields of a layer's launch; the caller adds what is its own (activations and their sizes,
// residual, second input, output pitch, ...)
ConvLaunch conv_launch(const ConvW &c, wsc_precision prec) {
    ConvLaunch L = {};
    L.w = c.w; L.s1 = c.s1; L.b1 = c.b1; L.s2 = c.s2; L.b2 = c.b2;
    L.Cin = c.Cin; L.Cout = c.Cout; L.CoutPad = c.CoutPad;
    L.kh = c.kh; L.kw = c.kw; L.stride = c.stride; L.pad = c.pad; L.relu = c.relu; L.dil = c.dil;
    L.form = c.form; L.prec = prec;
    return L;
}
// ... and on the zero-padded input of a CONV_FORM_STEM_ROWS layer: the buffer's own size, no padding left to apply
void on_padded_input(ConvLaunch &L, int in_h, int in_w) {
    L.H = in_h; L.W = in_w; L.pad = 0;
}

// (in2: the buffer of a 1x1 layer's second input, read at pixel stride `stride2`)
int add_conv_op(wsc_net *net, const std::string &label, const ConvW &c, int in, int out, int res, int in2 = -1, int stride2 = 0) {
    net->convs.push_back(c);
    Op op;
    op.label = label;
    op.type = OP_CONV; op.conv = (int)net->convs.size() - 1; op.in = in; op.out = out; op.res = res; op.in2 = in2; op.ps = stride2;
    net->ops.push_back(op);
    return WSC_OK;
}
// (pad: POOL_TORCH only)
void add_pool_op(wsc_net *net, PoolRule rule, int k, int stride, int pad, bool avg, int in, int out) {
    Op op;
    int n_pools = 0;
    for (const Op &o : net->ops) n_pools += o.type == OP_POOL;
    op.label = "pool:" + std::to_string(n_pools);
    op.type = OP_POOL; op.in = in; op.out = out; op.rule = rule; op.pk = k; op.ps = stride; op.pp = pad; op.avg = avg;
    net->ops.push_back(op);
}
// pixels (ho * stride, wo * stride) of `in` into channels [coff, coff + its channels) of `out`, a tensor of `pitch` channels
void add_gather_op(wsc_net *net, const std::string &label, int stride, int in, int out, int pitch, int coff) {
    Op op;
    op.label = label;
    op.type = OP_GATHER; op.in = in; op.out = out; op.ps = stride; op.pitch = pitch; op.coff = coff;
    net->ops.push_back(op);
}

// ResNet conv (bias-free) + FixedBatchNorm.
int resnet_conv(wsc_net *net, const Dict &d, const std::string &conv, const std::string &bn, int stride, int pad,
                int relu, ConvForm form, int in, int out, int res) {
    const HostTensor *w;
    WSC_TRY(get(d, conv + ".weight", 4, &w));
    std::vector<float> s, b;
    WSC_TRY(fold_bn(d, bn, (int)w->shape[0], 1e-5, s, b));
    ConvW c;
    WSC_TRY(make_conv(net, w, stride, pad, relu, form, s, b, nullptr, nullptr, &c));
    return add_conv_op(net, conv, c, in, out, res);
}

int build_resnet50_backbone(wsc_net *net, const Dict &d) {
    // stem: conv1 7x7 s2 p3 + bn1 + relu, maxpool 3x3 s2 p1          (resnet50.py:62-64, 96-99)
    // (f16x3: the padded-input form, staged like every other layer of that mode)
    WSC_TRY(resnet_conv(net, d, "resnet50.conv1", "resnet50.bn1", 2, 3, 1, conv_split(net->prec) == 2 ? CONV_FORM_STEM_ROWS : CONV_FORM_SMALL4, -1, 0, -1));
    add_pool_op(net, POOL_TORCH, 3, 2, 1, false, 0, 1);
    net->taps.push_back((int)net->ops.size() - 1); // stage1 = conv1, bn1, relu, maxpool (resnet50_irn.py:15)
    int cur = 1;
    const int blocks[4] = {3, 4, 6, 3};
    const int strides[4] = {1, 2, 2, 1}; // resnet50_cam.py:15 strides=(2,2,2,1): [0] is the stem
    for (int L = 0; L < 4; ++L) {
        for (int bi = 0; bi < blocks[L]; ++bi) {
            const std::string pre = "resnet50.layer" + std::to_string(L + 1) + "." + std::to_string(bi);
            const int s = bi == 0 ? strides[L] : 1;
            int f[3], nf = 0;
            for (int i = 0; i < 4 && nf < 3; ++i)
                if (i != cur) f[nf++] = i;
            // Bottleneck.forward, resnet50.py:34-54; the stride sits on conv2 (resnet50.py:24)
            WSC_TRY(resnet_conv(net, d, pre + ".conv1", pre + ".bn1", 1, 0, 1, CONV_FORM_GENERIC, cur, f[0], -1));
            bool fuse_here = false;
            // (WSC_PREC_F32 keeps the reference's operations: the projection is its own conv and conv3 adds it as a residual --
            // folding the two BatchNorm scales into one weight matrix rounds every weight once more, which is not the
            // reference's arithmetic and does not commute with powers of two moved between a BatchNorm and its neighbours)
            if (net->prec != WSC_PREC_F32 && has(d, pre + ".downsample.0.weight") && has(d, pre + ".conv3.weight")) {
                // (only for the shapes the concatenated GEMM takes: 1x1 kernels, K1 + K2 a multiple of the 64-channel K chunk;
                // anything else keeps the separate projection conv + residual)
                const HostTensor *w3, *wd;
                WSC_TRY(get(d, pre + ".conv3.weight", 4, &w3));
                WSC_TRY(get(d, pre + ".downsample.0.weight", 4, &wd));
                fuse_here = wd->shape[0] == w3->shape[0] && w3->shape[2] == 1 && w3->shape[3] == 1 && wd->shape[2] == 1 &&
                            wd->shape[3] == 1 && w3->shape[1] % 8 == 0 && wd->shape[1] % 8 == 0 &&
                            (w3->shape[1] + wd->shape[1]) % 64 == 0;
            }
            if (fuse_here) {
                // out = relu(bn3(conv3(y2)) + bn_d(conv_d(x)))  (resnet50.py:44-52) as ONE 1x1 conv over the concatenated channels
                // [y2 | x at the block's stride]: conv2 writes its channel range of that tensor, the shortcut input is gathered
                // beside it, and the two BatchNorm scales go into the weights -- relative to sigma_c = max(|s3_c|, |sd_c|), which
                // stays in the epilogue, so that neither branch's weights leave the half range (W3 * s3/sigma | Wd * sd/sigma,
                // shift b3 + bd).  The projection's output (215 MB per plane in layer1 at 64 samples) is never written or re-read
                // as a residual, and the stage's first block has one epilogue instead of two.
                const HostTensor *w3, *wd;
                WSC_TRY(get(d, pre + ".conv3.weight", 4, &w3));
                WSC_TRY(get(d, pre + ".downsample.0.weight", 4, &wd));
                const int Co = (int)w3->shape[0], K1 = (int)w3->shape[1], K2 = (int)wd->shape[1];
                std::vector<float> s3, b3, sd, bd;
                WSC_TRY(fold_bn(d, pre + ".bn3", Co, 1e-5, s3, b3));
                WSC_TRY(fold_bn(d, pre + ".downsample.1", Co, 1e-5, sd, bd));
                std::vector<float> wc((size_t)Co * (K1 + K2)), sig(Co), sh(Co);
                for (int co = 0; co < Co; ++co) {
                    float g = std::max(std::fabs(s3[co]), std::fabs(sd[co]));
                    if (!(g > 0.f)) g = 1.f;
                    sig[co] = g;
                    sh[co] = b3[co] + bd[co];
                    for (int k = 0; k < K1; ++k) wc[(size_t)co * (K1 + K2) + k] = w3->data[(size_t)co * K1 + k] * (s3[co] / g);
                    for (int k = 0; k < K2; ++k) wc[(size_t)co * (K1 + K2) + K1 + k] = wd->data[(size_t)co * K2 + k] * (sd[co] / g);
                }
                HostTensor wt;
                wt.data = wc.data(); wt.ndim = 4; wt.shape[0] = Co; wt.shape[1] = K1 + K2; wt.shape[2] = 1; wt.shape[3] = 1;
                WSC_TRY(resnet_conv(net, d, pre + ".conv2", pre + ".bn2", s, 1, 1, CONV_FORM_GENERIC, f[0], f[1], -1));
                ConvW c;
                WSC_TRY(make_conv(net, &wt, 1, 0, 1, CONV_FORM_GENERIC, sig, sh, nullptr, nullptr, &c));
                if (conv_split(net->prec) != 1) {
                    // the kernel reads the two inputs where they are: channel chunks [0, K1) from conv2's output, the rest from
                    // the block input at the block's stride (conv_igemm.hip, second A source)
                    WSC_TRY(add_conv_op(net, pre + ".conv3+downsample", c, f[1], f[0], -1, cur, s));
                } else {
                    // bf16x3 (three K segments per source): the concatenated tensor is materialised -- conv2 writes its channel
                    // range, the shortcut input is gathered beside it
                    net->ops.back().pitch = K1 + K2;
                    net->ops.back().coff = 0;
                    add_gather_op(net, pre + ".gather", s, cur, f[1], K1 + K2, K1);
                    WSC_TRY(add_conv_op(net, pre + ".conv3+downsample", c, f[1], f[0], -1));
                }
                cur = f[0];
                continue;
            }
            WSC_TRY(resnet_conv(net, d, pre + ".conv2", pre + ".bn2", s, 1, 1, CONV_FORM_GENERIC, f[0], f[1], -1));
            int res = cur;
            if (has(d, pre + ".downsample.0.weight")) {
                WSC_TRY(resnet_conv(net, d, pre + ".downsample.0", pre + ".downsample.1", s, 0, 0, CONV_FORM_GENERIC, cur, f[2], -1));
                res = f[2];
            }
            WSC_TRY(resnet_conv(net, d, pre + ".conv3", pre + ".bn3", 1, 0, 1, CONV_FORM_GENERIC, f[1], f[0], res));
            cur = f[0];
        }
        net->taps.push_back((int)net->ops.size() - 1); // stage L+2 = layer L+1
    }
    net->final_buf = cur;
    return WSC_OK;
}

int build_resnet50(wsc_net *net, const Dict &d) {
    WSC_TRY(build_resnet50_backbone(net, d));
    // CAM head: F.conv2d(x, classifier.weight), resnet50_cam.py:65 (ReLU + flip-add are a separate kernel)
    const HostTensor *cw;
    WSC_TRY(get(d, "classifier.weight", 4, &cw));
    WSC_CHECK(cw->shape[0] == net->C && cw->shape[2] == 1 && cw->shape[3] == 1, WSC_ERR_SHAPE,
              "classifier.weight must be [%d][F][1][1]", net->C);
    net->F = (int)cw->shape[1];
    std::vector<float> one(net->C, 1.f), zero(net->C, 0.f);
    WSC_TRY(make_conv(net, cw, 1, 0, 0, CONV_FORM_GENERIC, one, zero, nullptr, nullptr, &net->head));
    return WSC_OK;
}

// The optional `pool_spec` tensor, float32 [n_pools][3]: row i = (window, stride, same) of the i-th MaxPooling2D in the order the
// pools occur -- what a Keras-side session's architecture file says (02_cues/demo.py:104-124 builds the model with
// model_from_json) where the torch port has MaxPool2d(2, 2).  *present = false without the key: the fixed architecture.
int read_pool_spec(const Dict &d, int n_pools, std::vector<PoolSpec> *spec, bool *present) {
    *present = has(d, "pool_spec");
    if (!*present) return WSC_OK;
    const HostTensor *t;
    WSC_TRY(get(d, "pool_spec", 2, &t));
    WSC_CHECK(t->shape[0] == n_pools && t->shape[1] == 3, WSC_ERR_SHAPE, "pool_spec must be [%d][3] (window, stride, same) for this arch, got [%lld][%lld]",
              n_pools, (long long)t->shape[0], (long long)t->shape[1]);
    for (int i = 0; i < n_pools; ++i) {
        const float *r = t->data + 3 * i;
        WSC_CHECK(r[0] == std::floor(r[0]) && r[1] == std::floor(r[1]) && r[2] == std::floor(r[2]), WSC_ERR_INVALID,
                  "pool_spec row %d: (%g, %g, %g) is not integral", i, (double)r[0], (double)r[1], (double)r[2]);
        const PoolSpec ps = {(int)r[0], (int)r[1], (int)r[2]};
        WSC_CHECK((ps.k == 2 || ps.k == 3) && (ps.stride == 1 || ps.stride == 2) && ps.stride <= ps.k && (ps.same == 0 || ps.same == 1),
                  WSC_ERR_INVALID, "pool_spec row %d: window %d (2 / 3), stride %d (1 / 2, <= window), same %d (0 / 1)", i, ps.k, ps.stride, ps.same);
        spec->push_back(ps);
    }
    return WSC_OK;
}

// VGG-style stacks of common_cnn.make_layers: cfg entries >0 = conv out channels, -1 = 'M', -2 = 'D'.  `pools`: the geometry of
// the 'M' entries in their order (a `pool_spec`), or null for MaxPool2d(2, 2).
int build_plain_stack(wsc_net *net, const Dict &d, const std::string &root,
                      const std::vector<std::pair<std::string, std::vector<int>>> &cfg, int *cur_io,
                      int *feat_channels, std::vector<int> *layer_taps = nullptr, const std::vector<PoolSpec> *pools = nullptr) {
    int cur = *cur_io;
    int in_ch = 3;
    bool first = true;
    size_t n_pool = 0;
    int n_drop = 0;
    for (const auto &layer : cfg) {
        int idx = 0;
        for (int v : layer.second) {
            if (v == -1) { // nn.MaxPool2d(2, 2), common_cnn.py:131-132 -- or the session's own MaxPooling2D
                const int out = (cur + 1) & 1;
                if (pools) {
                    WSC_CHECK(n_pool < pools->size(), WSC_ERR_INVALID, "internal: pool_spec has %d rows, the stack more pools", (int)pools->size());
                    const PoolSpec &ps = (*pools)[n_pool++];
                    add_pool_op(net, ps.rule(), ps.k, ps.stride, 0, false, cur, out);
                } else add_pool_op(net, POOL_TORCH, 2, 2, 0, false, cur, out);
                cur = out;
                idx += 1;
            } else if (v == -2) { // nn.Dropout: identity in eval(); a site of wsc_net_forward_cls_train_drop
                // (numbered in table order; one behind a pool -- the IRN flavour of M7 -- belongs to no training pass)
                if (!net->ops.empty() && net->ops.back().type == OP_CONV) net->ops.back().drop_site = n_drop;
                n_drop += 1;
                idx += 1;
            } else {
                const std::string key = root + "." + layer.first + "." + std::to_string(idx);
                const HostTensor *w, *bias;
                WSC_TRY(get(d, key + ".weight", 4, &w));
                WSC_TRY(get(d, key + ".bias", 1, &bias));
                WSC_CHECK(w->shape[0] == v && w->shape[1] == in_ch && w->shape[2] == 3 && w->shape[3] == 3,
                          WSC_ERR_SHAPE, "'%s.weight' must be [%d][%d][3][3]", key.c_str(), v, in_ch);
                std::vector<float> one(v, 1.f), bb(bias->data, bias->data + v);
                const std::string bn = root + "." + layer.first + "." + std::to_string(idx + 2);
                ConvW c;
                if (has(d, bn + ".running_mean")) { // conv -> ReLU -> BatchNorm(eps=1e-3): common_cnn.py:138
                    std::vector<float> s2, b2;
                    WSC_TRY(fold_bn(d, bn, v, 1e-3, s2, b2));
                    WSC_TRY(make_conv(net, w, 1, 1, 1, first ? CONV_FORM_SMALL2 : CONV_FORM_GENERIC, one, bb, &s2, &b2, &c));
                    PlainBn pb; // (fold_bn has checked the tensors)
                    pb.name = bn; pb.C = v;
                    if (has(d, bn + ".eps") && d.at(bn + ".eps").data) pb.eps_fold = pb.eps = d.at(bn + ".eps").data[0];
                    WSC_TRY(upload(net, d.at(bn + ".weight").data, v * sizeof(float), (void **)&pb.gamma));
                    WSC_TRY(upload(net, d.at(bn + ".bias").data, v * sizeof(float), (void **)&pb.beta));
                    c.bn = (int)net->bns.size();
                    net->bns.push_back(pb);
                    idx += 3;
                } else {
                    WSC_TRY(make_conv(net, w, 1, 1, 1, first ? CONV_FORM_SMALL2 : CONV_FORM_GENERIC, one, bb, nullptr, nullptr, &c));
                    idx += 2;
                }
                const int in = first ? -1 : cur;
                const int out = first ? 0 : ((cur + 1) & 1);
                WSC_TRY(add_conv_op(net, key, c, in, out, -1));
                cur = out;
                in_ch = v;
                first = false;
            }
        }
        if (layer_taps) layer_taps->push_back((int)net->ops.size() - 1); // output of this layer
    }
    *cur_io = cur;
    *feat_channels = in_ch;
    return WSC_OK;
}

// optional per-class bias of a Grad-CAM head (`gradcam_bias`, C values): the Keras drivers contract alpha with the
// PRE-BatchNorm activation; on the post-BN feature map that is a head with weights alpha / s and this bias
// (wsscam/net/common.py::pre_bn_head).
int gradcam_bias(const Dict &d, int C, std::vector<float> &bias) {
    bias.assign(C, 0.f);
    if (!has(d, "gradcam_bias")) return WSC_OK;
    const HostTensor *gb;
    WSC_TRY(get(d, "gradcam_bias", 1, &gb));
    WSC_CHECK(gb->shape[0] == C, WSC_ERR_SHAPE, "gradcam_bias must be [%d]", C);
    for (int c = 0; c < C; ++c) bias[c] = gb->data[c];
    return WSC_OK;
}

// vgg16.py:44
const std::vector<std::pair<std::string, std::vector<int>>> VGG16_CFG = {{"layer1", {64, 64, -1}},
                                                                         {"layer2", {128, 128, -1}},
                                                                         {"layer3", {256, 256, 256, -1}},
                                                                         {"layer4", {512, 512, 512, 512, 512, 512}},
                                                                         {"layer5", {1024, -2, 1024, -2}}};

int build_vgg16(wsc_net *net, const Dict &d) {
    int cur = 0;
    std::vector<PoolSpec> pools;
    bool spec;
    WSC_TRY(read_pool_spec(d, 3, &pools, &spec));
    WSC_TRY(build_plain_stack(net, d, "vgg16", VGG16_CFG, &cur, &net->F, nullptr, spec ? &pools : nullptr));
    net->final_buf = cur;
    const HostTensor *lw;
    WSC_TRY(get(d, "vgg16.classifier.0.weight", 2, &lw));
    WSC_CHECK(lw->shape[0] >= net->C && lw->shape[1] == net->F, WSC_ERR_SHAPE,
              "vgg16.classifier.0.weight must be [>=%d][%d]", net->C, net->F);
    // CAM head = the Linear weight as a 1x1 kernel: vgg16_cam.py:48 -- or, when the state dict carries
    // `gradcam_weights` (F x C), the Grad-CAM alpha of 02_cues/utilities.py:60-99 (einsum 'ijkl,lm->ijkm')
    HostTensor hw = *lw;
    hw.ndim = 4; hw.shape[0] = net->C; hw.shape[2] = 1; hw.shape[3] = 1;
    std::vector<float> one(net->C, 1.f), zero(net->C, 0.f);
    std::vector<float> wt;
    if (has(d, "gradcam_weights")) {
        const HostTensor *gw;
        WSC_TRY(get(d, "gradcam_weights", 2, &gw));
        WSC_CHECK(gw->shape[0] == net->F && gw->shape[1] == net->C, WSC_ERR_SHAPE,
                  "gradcam_weights must be [%d][%d]", net->F, net->C);
        wt.resize((size_t)net->C * net->F);
        for (int f = 0; f < net->F; ++f)
            for (int c = 0; c < net->C; ++c) wt[(size_t)c * net->F + f] = gw->data[(size_t)f * net->C + c];
        hw.data = wt.data();
        WSC_TRY(gradcam_bias(d, net->C, zero));
    } else net->head_is_cls = true;
    WSC_TRY(make_conv(net, &hw, 1, 0, 0, CONV_FORM_GENERIC, one, zero, nullptr, nullptr, &net->head));
    net->Ccls = net->C;
    net->cls_max = 0;
    WSC_TRY(upload(net, lw->data, (size_t)net->C * net->F * sizeof(float), (void **)&net->cls_w));
    if (has(d, "vgg16.classifier.0.bias")) {
        const HostTensor *lb;
        WSC_TRY(get(d, "vgg16.classifier.0.bias", 1, &lb));
        WSC_TRY(upload(net, lb->data, (size_t)net->C * sizeof(float), (void **)&net->cls_b));
    }
    return WSC_OK;
}

int build_m7(wsc_net *net, const Dict &d) {
    const std::vector<std::pair<std::string, std::vector<int>>> cfg = {
        {"layer1", {64, 64, -1}}, {"layer2", {128, 128, -1}}, {"layer3_p1", {256, 256, 256}}}; // m7.py:41
    int cur = 0;
    std::vector<PoolSpec> pools; // the two of the stack, then layer3_p2 of the classifier branch
    WSC_TRY(read_pool_spec(d, 3, &pools, &net->cls_pool_set));
    if (net->cls_pool_set) net->cls_pool = pools[2];
    WSC_TRY(build_plain_stack(net, d, "m7", cfg, &cur, &net->F, nullptr, net->cls_pool_set ? &pools : nullptr));
    net->final_buf = cur;
    // Grad-CAM weights (F x C) transposed as the 1x1 head: m7_cam.py:45-46
    const HostTensor *gw;
    WSC_TRY(get(d, "gradcam_weights", 2, &gw));
    WSC_CHECK(gw->shape[0] == net->F && gw->shape[1] == net->C, WSC_ERR_SHAPE, "gradcam_weights must be [%d][%d]",
              net->F, net->C);
    std::vector<float> wt((size_t)net->C * net->F);
    for (int f = 0; f < net->F; ++f)
        for (int c = 0; c < net->C; ++c) wt[(size_t)c * net->F + f] = gw->data[(size_t)f * net->C + c];
    HostTensor hw;
    hw.data = wt.data(); hw.ndim = 4; hw.shape[0] = net->C; hw.shape[1] = net->F; hw.shape[2] = 1; hw.shape[3] = 1;
    std::vector<float> one(net->C, 1.f), zero(net->C, 0.f);
    WSC_TRY(gradcam_bias(d, net->C, zero));
    WSC_TRY(make_conv(net, &hw, 1, 0, 0, CONV_FORM_GENERIC, one, zero, nullptr, nullptr, &net->head));
    // classifier branch: layer3_p2 (MaxPool 2x2 + Dropout) -> AdaptiveMaxPool2d(1) -> Linear + Sigmoid
    // (m7_cam.py:32-35).  max over 2x2-pooled map == global max when h, w are even.  With a `pool_spec` the pool is its third
    // row and run_classifier takes the maximum of the pooled map where the two differ.
    const HostTensor *lw;
    WSC_TRY(get(d, "m7.classifier.0.weight", 2, &lw));
    WSC_CHECK(lw->shape[0] >= net->C && lw->shape[1] == net->F, WSC_ERR_SHAPE,
              "m7.classifier.0.weight must be [>=%d][%d]", net->C, net->F);
    net->Ccls = net->C;
    net->cls_max = 1;
    WSC_TRY(upload(net, lw->data, (size_t)net->C * net->F * sizeof(float), (void **)&net->cls_w));
    if (has(d, "m7.classifier.0.bias")) {
        const HostTensor *lb;
        WSC_TRY(get(d, "m7.classifier.0.bias", 1, &lb));
        WSC_TRY(upload(net, lb->data, (size_t)net->C * sizeof(float), (void **)&net->cls_b));
    }
    return WSC_OK;
}

// ---- IRNet EdgeDisplacement heads (resnet50_irn.py:22-92, vgg16_irn.py:28-98) -----------------------------
struct HeadSpec {
    const char *name;
    int src, stride, cout, groups, up, dst, coff;
};

// Conv2d(Cin, Cout, 1, bias=False) weights `<name>.0.weight`, GroupNorm affine `<name>.1.{weight,bias}`
int add_irn_head(wsc_net *net, const Dict &d, const HeadSpec &hs) {
    const HostTensor *w, *g, *b;
    const std::string nm = hs.name;
    WSC_TRY(get(d, nm + ".0.weight", 4, &w));
    WSC_TRY(get(d, nm + ".1.weight", 1, &g));
    WSC_TRY(get(d, nm + ".1.bias", 1, &b));
    WSC_CHECK(w->shape[0] == hs.cout && w->shape[2] == 1 && w->shape[3] == 1 && g->shape[0] == hs.cout &&
                  b->shape[0] == hs.cout,
              WSC_ERR_SHAPE, "'%s': expected a 1x1 conv with %d outputs + GroupNorm", hs.name, hs.cout);
    IrnHead h;
    h.name = nm;
    std::vector<float> one(hs.cout, 1.f), zero(hs.cout, 0.f);
    WSC_TRY(make_conv(net, w, hs.stride, 0, 0, CONV_FORM_GENERIC, one, zero, nullptr, nullptr, &h.conv));
    h.groups = hs.groups; h.up = hs.up; h.src = hs.src; h.dst = hs.dst; h.coff = hs.coff;
    WSC_TRY(upload(net, g->data, sizeof(float) * hs.cout, (void **)&h.gamma));
    WSC_TRY(upload(net, b->data, sizeof(float) * hs.cout, (void **)&h.beta));
    net->heads.push_back(h);
    return WSC_OK;
}

int build_irn_heads(wsc_net *net, const Dict &d, const std::vector<HeadSpec> &specs, const std::vector<IrnCat> &cats,
                    const std::string &edge_final, int edge_in, const std::string &dp_final) {
    net->cats = cats;
    net->edge_final = edge_final; net->dp_final = dp_final; net->edge_in = edge_in;
    for (const HeadSpec &hs : specs) WSC_TRY(add_irn_head(net, d, hs));
    // final edge conv = Conv2d(edge_in, 1, 1, bias=True) on the edge concat, zero-padded to cats[0].channels inputs
    const HostTensor *w6, *b6, *w7;
    WSC_TRY(get(d, edge_final + ".weight", 4, &w6));
    WSC_TRY(get(d, edge_final + ".bias", 1, &b6));
    WSC_CHECK(w6->shape[0] == 1 && w6->shape[1] == edge_in, WSC_ERR_SHAPE, "%s.weight must be [1][%d][1][1]",
              edge_final.c_str(), edge_in);
    const int cin_pad = cats[0].channels;
    std::vector<float> w6p(cin_pad, 0.f);
    for (int i = 0; i < edge_in; ++i) w6p[i] = w6->data[i];
    HostTensor t6;
    t6.data = w6p.data(); t6.ndim = 4; t6.shape[0] = 1; t6.shape[1] = cin_pad; t6.shape[2] = 1; t6.shape[3] = 1;
    std::vector<float> one1(1, 1.f), bias1(1, b6->data[0]);
    WSC_TRY(make_conv(net, &t6, 1, 0, 0, CONV_FORM_GENERIC, one1, bias1, nullptr, nullptr, &net->edge6));
    // final displacement conv = Conv2d(256, 2, 1, bias=False); MeanShift subtracts running_mean in eval
    // (resnet50_irn.py:96-108)
    WSC_TRY(get(d, dp_final + ".weight", 4, &w7));
    WSC_CHECK(w7->shape[0] == 2 && w7->shape[1] == cats.back().channels, WSC_ERR_SHAPE, "%s.weight must be [2][%d][1][1]",
              dp_final.c_str(), cats.back().channels);
    std::vector<float> one2(2, 1.f), zero2(2, 0.f);
    WSC_TRY(make_conv(net, w7, 1, 0, 0, CONV_FORM_GENERIC, one2, zero2, nullptr, nullptr, &net->dp7b));
    if (has(d, "mean_shift.running_mean")) {
        const HostTensor *ms;
        WSC_TRY(get(d, "mean_shift.running_mean", 1, &ms));
        WSC_CHECK(ms->shape[0] == 2, WSC_ERR_SHAPE, "mean_shift.running_mean must have 2 entries");
        net->mean_shift[0] = ms->data[0];
        net->mean_shift[1] = ms->data[1];
    }
    return WSC_OK;
}

// HeadSpec: {name, src, conv stride, out channels, GroupNorm groups, upsample, dst concat, channel offset};
// src > 0 is a backbone stage, src < 0 the concat buffer -src - 1.
// ResNet50 / VGG16 concat buffers: 0 = edge concat (5 x 32 -> 192 ch), 1 = dp3|dp4|dp5 (768, stage-3 resolution),
// 2 = dp1|dp2|dp_up3 (448), 3 = fc_dp7 hidden (256); all but 1 at the stage-2 resolution.
const std::vector<IrnCat> IRN_CATS5 = {{192, 2, 1}, {768, 3, 1}, {448, 2, 1}, {256, 2, 1}};

int build_resnet50_irn(wsc_net *net, const Dict &d) {
    WSC_TRY(build_resnet50_backbone(net, d));
    const std::vector<HeadSpec> specs = {
        {"fc_edge1", 1, 1, 32, 4, 1, 0, 0},   {"fc_edge2", 2, 1, 32, 4, 1, 0, 32},  {"fc_edge3", 3, 1, 32, 4, 2, 0, 64},
        {"fc_edge4", 4, 1, 32, 4, 4, 0, 96},  {"fc_edge5", 5, 1, 32, 4, 4, 0, 128}, {"fc_dp1", 1, 1, 64, 8, 1, 2, 0},
        {"fc_dp2", 2, 1, 128, 16, 1, 2, 64},  {"fc_dp3", 3, 1, 256, 16, 1, 1, 0},   {"fc_dp4", 4, 1, 256, 16, 2, 1, 256},
        {"fc_dp5", 5, 1, 256, 16, 2, 1, 512}, {"fc_dp6", -2, 1, 256, 16, 2, 2, 192}, {"fc_dp7", -3, 1, 256, 16, 1, 3, 0}};
    return build_irn_heads(net, d, specs, IRN_CATS5, "fc_edge6", 160, "fc_dp7.3");
}

int build_vgg16_irn(wsc_net *net, const Dict &d) {
    int cur = 0;
    WSC_TRY(build_plain_stack(net, d, "vgg16", VGG16_CFG, &cur, &net->F, &net->taps)); // stage k = layer k (vgg16_irn.py:21-25)
    net->final_buf = cur;
    // ds_fac = 0.25 (vgg16_irn.py:30-98): stage1 is at 1/2 resolution and its heads use a stride-2 1x1 conv
    const std::vector<HeadSpec> specs = {
        {"fc_edge1", 1, 2, 32, 4, 1, 0, 0},   {"fc_edge2", 2, 1, 32, 4, 1, 0, 32},  {"fc_edge3", 3, 1, 32, 4, 2, 0, 64},
        {"fc_edge4", 4, 1, 32, 4, 2, 0, 96},  {"fc_edge5", 5, 1, 32, 4, 2, 0, 128}, {"fc_dp1", 1, 2, 64, 8, 1, 2, 0},
        {"fc_dp2", 2, 1, 128, 16, 1, 2, 64},  {"fc_dp3", 3, 1, 256, 16, 1, 1, 0},   {"fc_dp4", 4, 1, 256, 16, 1, 1, 256},
        {"fc_dp5", 5, 1, 256, 16, 1, 1, 512}, {"fc_dp6", -2, 1, 256, 16, 2, 2, 192}, {"fc_dp7", -3, 1, 256, 16, 1, 3, 0}};
    return build_irn_heads(net, d, specs, IRN_CATS5, "fc_edge6", 160, "fc_dp7.3");
}

// m7_irn.py:19-21,24-69,96-112: three stages (layer1 @1/2, layer2 @1/4, layer3_p1 + layer3_p2 @1/8); the edge
// branch ends at the stage-1 resolution (1/2), the displacement branch at 1/4; fc_dp4 is a head on fc_dp3's output.
int build_m7_irn(wsc_net *net, const Dict &d) {
    const std::vector<std::pair<std::string, std::vector<int>>> cfg = {
        {"layer1", {64, 64, -1}}, {"layer2", {128, 128, -1}}, {"layer3_p1", {256, 256, 256}}, {"layer3_p2", {-1, -2}}};
    int cur = 0;
    std::vector<int> layer_taps;
    WSC_TRY(build_plain_stack(net, d, "m7", cfg, &cur, &net->F, &layer_taps));
    net->final_buf = cur;
    net->taps = {layer_taps[0], layer_taps[1], layer_taps[3]};
    const std::vector<IrnCat> cats = {{128, 1, 1}, {256, 3, 1}, {448, 2, 1}, {256, 2, 1}}; // edge | dp3 | dp1|dp2|dp4 | hidden
    const std::vector<HeadSpec> specs = {
        {"fc_edge1", 1, 1, 32, 4, 1, 0, 0},  {"fc_edge2", 2, 1, 32, 4, 2, 0, 32},  {"fc_edge3", 3, 1, 32, 4, 4, 0, 64},
        {"fc_dp1", 1, 2, 64, 8, 1, 2, 0},    {"fc_dp2", 2, 1, 128, 16, 1, 2, 64},  {"fc_dp3", 3, 1, 256, 16, 1, 1, 0},
        {"fc_dp4", -2, 1, 256, 16, 2, 2, 192}, {"fc_dp5", -3, 1, 256, 16, 1, 3, 0}};
    return build_irn_heads(net, d, specs, cats, "fc_edge4", 96, "fc_dp5.3");
}

// ---- DeepLab-VGG16 of 03a_sec-dsrg (SEC.py:117-128,150-218 / DSRG.py:169-186,203-295) ----------------------------------
// `<layer>.w` is TensorFlow's HWIO [kh][kw][Cin][Cout], `<layer>.b` [Cout].  A missing or mis-shaped tensor is WSC_ERR_SHAPE
// with the layer's name.  Every layer is conv + bias + ReLU except fc8; dropout is the identity (drop_prob = 0).
int deeplab_conv(wsc_net *net, const Dict &d, const std::string &layer, int k, int in_ch, int want_cout, int dil, int relu,
                 ConvForm form, ConvW *out) {
    auto wi = d.find(layer + ".w"), bi = d.find(layer + ".b");
    WSC_CHECK(wi != d.end() && wi->second.data != nullptr && bi != d.end() && bi->second.data != nullptr, WSC_ERR_SHAPE,
              "layer '%s': '%s.w' / '%s.b' missing", layer.c_str(), layer.c_str(), layer.c_str());
    const HostTensor &w = wi->second, &b = bi->second;
    WSC_CHECK(w.ndim == 4 && w.shape[0] == k && w.shape[1] == k && w.shape[2] == in_ch && w.shape[3] >= 1, WSC_ERR_SHAPE,
              "layer '%s': '.w' must be HWIO [%d][%d][%d][Cout], got ndim %d [%lld][%lld][%lld][%lld]", layer.c_str(), k, k, in_ch, w.ndim,
              (long long)w.shape[0], (long long)w.shape[1], (long long)w.shape[2], (long long)w.shape[3]);
    const int Cout = (int)w.shape[3];
    WSC_CHECK(want_cout > 0 ? Cout == want_cout : Cout % 64 == 0, WSC_ERR_SHAPE,
              "layer '%s': %d output channels (%s)", layer.c_str(), Cout, want_cout > 0 ? "the class count is expected" : "a multiple of 64 is needed");
    WSC_CHECK(b.numel() == Cout, WSC_ERR_SHAPE, "layer '%s': '.b' has %lld entries for %d output channels", layer.c_str(),
              (long long)b.numel(), Cout);
    std::vector<float> oihw((size_t)Cout * in_ch * k * k);
    for (int r = 0; r < k; ++r)
        for (int q = 0; q < k; ++q)
            for (int ci = 0; ci < in_ch; ++ci)
                for (int co = 0; co < Cout; ++co)
                    oihw[(((size_t)co * in_ch + ci) * k + r) * k + q] = w.data[(((size_t)r * k + q) * in_ch + ci) * Cout + co];
    HostTensor t;
    t.data = oihw.data(); t.ndim = 4; t.shape[0] = Cout; t.shape[1] = in_ch; t.shape[2] = k; t.shape[3] = k;
    std::vector<float> one(Cout, 1.f), bias(b.data, b.data + Cout);
    // TF SAME for an odd kernel at stride 1: pad = dil (k - 1) / 2 on every side
    WSC_TRY(make_conv(net, &t, 1, dil * (k - 1) / 2, relu, form, one, bias, nullptr, nullptr, out));
    out->dil = dil;
    return WSC_OK;
}

int build_deeplab(wsc_net *net, const Dict &d, bool aspp) {
    // {layer, dilation}; "" = a pool: 2 / 1 = max at that stride, 0 = the 3x3 average pool5a
    struct Item { const char *name; int v; };
    const Item trunk[] = {{"conv1_1", 1}, {"conv1_2", 1}, {"", 2}, {"conv2_1", 1}, {"conv2_2", 1}, {"", 2},
                          {"conv3_1", 1}, {"conv3_2", 1}, {"conv3_3", 1}, {"", 2}, {"conv4_1", 1}, {"conv4_2", 1}, {"conv4_3", 1}, {"", 1},
                          {"conv5_1", 2}, {"conv5_2", 2}, {"conv5_3", 2}, {"", 1}, {"", 0}};
    int cur = 0, in_ch = 3;
    bool first = true;
    for (const Item &it : trunk) {
        if (it.name[0] == 0) {
            const int out = (cur + 1) & 1;
            add_pool_op(net, POOL_TF_SAME, 3, it.v == 0 ? 1 : it.v, 0, it.v == 0, cur, out);
            cur = out;
            continue;
        }
        ConvW c;
        WSC_TRY(deeplab_conv(net, d, it.name, 3, in_ch, 0, it.v, 1, first ? CONV_FORM_SMALL2 : CONV_FORM_GENERIC, &c));
        const int out = first ? 0 : ((cur + 1) & 1);
        WSC_TRY(add_conv_op(net, it.name, c, first ? -1 : cur, out, -1));
        cur = out;
        in_ch = c.Cout;
        first = false;
    }
    net->final_buf = cur;
    net->F = in_ch;
    const int rates_aspp[4] = {6, 12, 18, 24};
    const int nb = aspp ? 4 : 1;
    for (int k = 0; k < nb; ++k) {
        const std::string sfx = aspp ? "_" + std::to_string(k + 1) : "";
        SegBranch br;
        WSC_TRY(deeplab_conv(net, d, "fc6" + sfx, 3, in_ch, 0, aspp ? rates_aspp[k] : 12, 1, CONV_FORM_GENERIC, &br.fc6));
        WSC_TRY(deeplab_conv(net, d, "fc7" + sfx, 1, br.fc6.Cout, 0, 1, 1, CONV_FORM_GENERIC, &br.fc7));
        WSC_TRY(deeplab_conv(net, d, "fc8" + sfx, 1, br.fc7.Cout, net->C, 1, 0, CONV_FORM_GENERIC, &br.fc8));
        net->seg.push_back(br);
    }
    return WSC_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct OpDims {
    int H, W, C;    // the op's input (Op::in) as the op finds it
    int Ho, Wo, Co; // its output; Co = all channels of the tensor it writes into (Op::pitch where set)
    int H2, W2, C2; // the second input (Op::in2), zeros without one
};
struct Plan {
    std::vector<OpDims> ops;
    size_t max_act = 0; // elements
    int hf = 0, wf = 0; // final feature map size
    size_t out_elems(int N, int op) const { return (size_t)N * ops[op].Ho * ops[op].Wo * ops[op].Co; }
};

// (SH x SW network input: square for the fixed-size configurations, the image's own size for outsize = None)
int plan_dims(const wsc_net *net, int N, int SH, int SW, Plan *pl);
int plan_dims(const wsc_net *net, int N, int S, Plan *pl) { return plan_dims(net, N, S, S, pl); }
int plan_dims(const wsc_net *net, int N, int SH, int SW, Plan *pl) {
    int bh[4] = {0, 0, 0, 0}, bw[4] = {0, 0, 0, 0}, bc[4] = {0, 0, 0, 0};
    pl->max_act = 0;
    for (const Op &op : net->ops) {
        OpDims d = {};
        d.H = op.in < 0 ? SH : bh[op.in]; d.W = op.in < 0 ? SW : bw[op.in]; d.C = op.in < 0 ? 4 : bc[op.in];
        if (op.type == OP_CONV) {
            const ConvW &c = net->convs[op.conv];
            d.Ho = (d.H + 2 * c.pad - ((c.kh - 1) * c.dil + 1)) / c.stride + 1;
            d.Wo = (d.W + 2 * c.pad - ((c.kw - 1) * c.dil + 1)) / c.stride + 1;
            d.Co = op.pitch ? op.pitch : c.Cout;
            if (op.in2 >= 0) {
                d.H2 = bh[op.in2]; d.W2 = bw[op.in2]; d.C2 = bc[op.in2];
                WSC_CHECK(c.kh == 1 && c.kw == 1 && c.stride == 1 && (d.H - 1) * op.ps < d.H2 && (d.W - 1) * op.ps < d.W2,
                          WSC_ERR_INVALID, "internal: second input of a %d x %d layer does not cover its %d x %d output", c.kh, c.kw, d.H, d.W);
            }
            WSC_CHECK(d.C + d.C2 == c.Cin, WSC_ERR_INVALID, "internal: channel mismatch %d vs %d", d.C + d.C2, c.Cin);
        } else if (op.type == OP_GATHER) {
            d.Ho = (d.H - 1) / op.ps + 1;
            d.Wo = (d.W - 1) / op.ps + 1;
            d.Co = op.pitch;
            WSC_CHECK(d.Ho == bh[op.out] && d.Wo == bw[op.out] && bc[op.out] == op.pitch && op.coff + d.C <= op.pitch, WSC_ERR_INVALID,
                      "internal: gather into a %d x %d x %d tensor does not fit", bh[op.out], bw[op.out], bc[op.out]);
        } else {
            PoolGeom g; // (a window wider than the map: Ho or Wo = 0, the check below)
            pool_geom(op.rule, op.pk, op.ps, op.pp, op.avg, d.H, d.W, &g);
            d.Ho = g.Ho; d.Wo = g.Wo; d.Co = d.C;
        }
        WSC_CHECK(d.Ho > 0 && d.Wo > 0, WSC_ERR_INVALID, "input size %d x %d too small for this network", SH, SW);
        bh[op.out] = d.Ho; bw[op.out] = d.Wo; bc[op.out] = d.Co;
        pl->ops.push_back(d);
        pl->max_act = std::max(pl->max_act, pl->out_elems(N, (int)pl->ops.size() - 1));
    }
    pl->hf = bh[net->final_buf];
    pl->wf = bw[net->final_buf];
    return WSC_OK;
}

// workspace bytes of the copies of the stage taps x1..x5 (run_backbone's `taps`)
size_t taps_bytes(const wsc_net *net, const Plan &pl, int N) {
    size_t b = 0;
    for (int op : net->taps) b += act_bytes(pl.out_elems(N, op), net->prec);
    return b;
}

// conv 7x7 / 2 / 3 (-> 64) + BN + ReLU followed by MaxPool 3 / 2 / 1 (resnet50.py:54-64) of the f16x3 padded-input stem: one kernel
// (stem_pool.hip), unless the conv's own output is wanted (a tap) or the path is switched off
bool stem_pool_fused(const wsc_ctx *ctx, const wsc_net *net) {
    if (net->ops.empty() || net->ops[0].type != OP_CONV || net->ops[0].in >= 0 || net->convs[net->ops[0].conv].form != CONV_FORM_STEM_ROWS)
        return false;
    const ConvW &c0 = net->convs[net->ops[0].conv];
    bool tapped = false;
    for (int tp : net->taps) tapped = tapped || tp == 0;
    return ctx->opt[WSC_OPT_STEM_POOL_FUSED] && net->ops.size() > 1 && net->ops[1].type == OP_POOL &&
           net->ops[1].in == net->ops[0].out && net->ops[1].rule == POOL_TORCH && !net->ops[1].avg && net->ops[1].pk == 3 &&
           net->ops[1].ps == 2 && net->ops[1].pp == 1 &&
           c0.kh == 7 && c0.kw == 7 && c0.stride == 2 && c0.pad == 3 && c0.Cout == 64 && c0.s2 == nullptr &&
           net->ops[0].res < 0 && conv_fmt(net->prec) == 1 && !tapped;
}

// wsc_net_forward_trace's observer: after op i, the tensor the op wrote into (all `Co` channels of it, OpDims) goes to
// out + off[i] as fp32 NHWC (launch_act_to_f32: hi + lo, the exact value the next op reads); off[i] < 0: not wanted
struct TraceSink {
    const long long *off;
    float *out;
};

// wsc_net_forward_cls_train's part of run_backbone: where op i's BatchNorm finds its input a (the trace copy of the conv's output)
// and leaves its statistics and the value the next op reads, all in the caller's tape; the running statistics (or null)
// the dropout of a training pass through a plain stack (wsc_net_forward_cls_train_drop / wsc_net_backward_cls_drop), drop_prob > 0
struct ClsDrop {
    float drop_prob;
    unsigned long long seed;
    unsigned step;
};
struct BnTrainSink {
    const long long *a_off, *stats_off, *y_off; // per op, floats into `tape`
    float *tape;
    float keep;
    int unbiased;
    float *run; // [2][C] per BatchNorm layer in stack order, or null
    const ClsDrop *drop; // null: every Op::drop_site is the identity
};
// a [M][C] -> the batch statistics; the activation `act` = the normalised output through the store the GroupNorm heads use (one
// "sample" of M pixels, every channel a group of its own: the same fmaf on the same float statistics, the planes' split and the
// range flag of every other activation store); the tape's entry = the fp32 value those planes hold
int bn_train_step(wsc_ctx *ctx, const wsc_net *net, const BnTrainSink &s, int op, long long M, Act act) {
    const PlainBn &bn = net->bns[net->convs[net->ops[op].conv].bn];
    const float *a = s.tape + s.a_off[op];
    float *stats = s.tape + s.stats_off[op], *run = nullptr;
    if (s.run) {
        run = s.run;
        for (int k = 0; k < net->convs[net->ops[op].conv].bn; ++k) run += 2 * net->bns[k].C;
    }
    WSC_TRY(launch_batch_norm_train(ctx, a, M, bn.C, bn.gamma, bn.beta, bn.eps, s.keep, s.unbiased, run, stats, nullptr));
    if (s.drop && net->ops[op].drop_site >= 0) // (one pass: the dropped value into the planes and into the tape)
        return launch_batch_norm_apply_drop(ctx, a, stats, bn.gamma, bn.beta, M, bn.C, act, s.tape + s.y_off[op], s.drop->drop_prob,
                                            s.drop->seed, s.drop->step, (unsigned)net->ops[op].drop_site);
    WSC_TRY(launch_group_norm_apply(ctx, a, stats, bn.gamma, bn.beta, 1, (int)M, 1, bn.C, bn.C, 1, 0, act, (int)M, 1, bn.C, 0));
    return launch_act_to_f32(ctx, act, (size_t)M * bn.C, s.tape + s.y_off[op]);
}

// Runs the conv stack on N samples; *feat is the final feature map.  *extra: `extra_bytes` of workspace for the caller.  With
// `taps` the stage outputs x1..x5 (net->taps) are copied to the start of that region, in stage order, and *extra is what
// follows them -- the rotating activation buffers are overwritten as the stack proceeds.
int run_backbone(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, size_t extra_bytes, Act *feat, int *hf, int *wf,
                 void **extra, std::vector<Act> *taps = nullptr, int SW = 0, bool nhwc_in = false, Act *spare = nullptr,
                 const TraceSink *trace = nullptr, Act *xin_out = nullptr, const BnTrainSink *bn_train = nullptr) {
    // (trace: copies between the launches, nothing else -- the launches are the ones of a run without it)
    // (bn_train: the training form of a plain stack -- a conv runs without its post-ReLU affine, and behind the trace copy of its
    // output the BatchNorm of the batch statistics rewrites the activation; a net without BatchNorm launches what it launches without)
    // (xin_out: the NHWC4 input activation the first op reads; no op writes it)
    // (spare: a rotating buffer other than *feat, free once the stack has run -- any tensor no larger than the feature map fits)
    // (nhwc_in: x_dev is [N][S][SW][3] instead of [N][3][S][SW] -- the DeepLab nets take TensorFlow's layout)
    if (SW <= 0) SW = S; // S x SW input (SW given for the non-square, native-size path)
    Plan pl;
    WSC_TRY(plan_dims(net, N, S, SW, &pl));
    // f16x3 stem (CONV_FORM_STEM_ROWS): the NHWC4 input carries its zero border
    int in_h = S, in_w = SW, in_pad = 0;
    bool fused_stem = false;
    if (!net->ops.empty() && net->ops[0].type == OP_CONV && net->ops[0].in < 0 && net->convs[net->ops[0].conv].form == CONV_FORM_STEM_ROWS) {
        const ConvW &c0 = net->convs[net->ops[0].conv];
        conv_stem_rows_input_dims(pl.ops[0].Ho, pl.ops[0].Wo, c0.stride, c0.kh, &in_h, &in_w);
        in_pad = c0.pad;
        fused_stem = stem_pool_fused(ctx, net);
        if (fused_stem) {
            stem_pool_input_dims(S, SW, &in_h, &in_w);
            in_pad = 5;
        }
    }
    const size_t in_elems = (size_t)N * in_h * in_w * 4;
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, act_bytes(in_elems, net->prec) + 4 * act_bytes(pl.max_act, net->prec) + align_up(extra_bytes, 256), &ws));
    char *p = (char *)ws;
    const Act xin = act_carve(p, in_elems, net->prec);
    Act buf[4];
    for (Act &b : buf) b = act_carve(p, pl.max_act, net->prec);
    if (taps)
        for (int op : net->taps) taps->push_back(act_carve(p, pl.out_elems(N, op), net->prec));
    *extra = (void *)p;

    if (nhwc_in) {
        WSC_CHECK(in_pad == 0, WSC_ERR_INVALID, "internal: an NHWC input has no padded-stem form");
        WSC_TRY(launch_nhwc3_to_nhwc4(ctx, x_dev, N, S, SW, xin));
    } else if (in_pad > 0) WSC_TRY(launch_nchw_to_nhwc4_pad(ctx, x_dev, N, S, SW, in_h, in_w, in_pad, xin, ctx->range_dev));
    else WSC_TRY(launch_nchw_to_nhwc4(ctx, x_dev, N, S, SW, xin, ctx->range_dev)); // (a net raises the flag in every precision)
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const Op &op = net->ops[i];
        const OpDims &d = pl.ops[i];
        const Act src = op.in < 0 ? xin : buf[op.in];
        if (fused_stem && i == 0) continue; // computed together with the pool that follows
        if (fused_stem && i == 1) {
            const ConvW &c0 = net->convs[net->ops[0].conv];
            WSC_TRY(launch_stem_pool(ctx, xin, N, S, SW, (const bf16_t *)c0.w, conv_k_layout(c0.kh, c0.kw, c0.Cin, c0.form, net->prec).Kw, c0.s1,
                                     c0.b1, c0.relu, buf[op.out]));
        } else if (op.type == OP_CONV) {
            const ConvW &c = net->convs[op.conv];
            ConvLaunch L = conv_launch(c, net->prec);
            L.x = src;
            if (op.res >= 0) L.res = buf[op.res];
            L.y = buf[op.out].at(op.coff);
            L.ldy = op.pitch; // (0: dense)
            if (op.in2 >= 0) {
                L.x2 = buf[op.in2];
                L.H2 = d.H2; L.W2 = d.W2; L.C2 = d.C2; L.stride2 = op.ps;
            }
            L.N = N; L.H = d.H; L.W = d.W; L.Ho = d.Ho; L.Wo = d.Wo;
            if (c.form == CONV_FORM_STEM_ROWS && op.in < 0) on_padded_input(L, in_h, in_w);
            if (bn_train) L.s2 = L.b2 = nullptr;
            WSC_TRY(conv_igemm_launch(ctx, L));
        } else if (op.type == OP_GATHER) {
            WSC_TRY(launch_gather_strided(ctx, src, N, d.H, d.W, d.C, op.ps, d.Ho, d.Wo, buf[op.out].at(op.coff), op.pitch));
        } else {
            PoolGeom g;
            WSC_CHECK(pool_geom(op.rule, op.pk, op.ps, op.pp, op.avg, d.H, d.W, &g), WSC_ERR_INVALID, "internal: a pool plan_dims let through");
            WSC_TRY(launch_pool(ctx, src, N, d.H, d.W, d.C, g, buf[op.out]));
        }
        // (a dropout site of a stack without BatchNorm: the post-ReLU value dropped in place of the copy, as behind fc6 / fc7)
        const bool relu_site = bn_train && bn_train->drop && op.type == OP_CONV && op.drop_site >= 0 && net->convs[op.conv].bn < 0;
        if (relu_site) {
            WSC_CHECK(trace && trace->off[i] >= 0 && op.pitch == 0, WSC_ERR_INVALID, "internal: a dropout site without its tape entry");
            WSC_TRY(launch_seg_dropout(ctx, buf[op.out], pl.out_elems(N, (int)i), d.Co, bn_train->drop->drop_prob, bn_train->drop->seed,
                                       bn_train->drop->step, (unsigned)op.drop_site, trace->out + trace->off[i]));
        } else if (trace && trace->off[i] >= 0) WSC_TRY(launch_act_to_f32(ctx, buf[op.out], pl.out_elems(N, (int)i), trace->out + trace->off[i]));
        if (bn_train && op.type == OP_CONV && net->convs[op.conv].bn >= 0)
            WSC_TRY(bn_train_step(ctx, net, *bn_train, (int)i, (long long)N * d.Ho * d.Wo, buf[op.out]));
        if (taps)
            for (size_t k = 0; k < net->taps.size(); ++k)
                if (net->taps[k] == (int)i) {
                    const size_t nb = pl.out_elems(N, (int)i) * conv_elem_bytes(net->prec);
                    WSC_HIP(hipMemcpyAsync((*taps)[k].hi, buf[op.out].hi, nb, hipMemcpyDeviceToDevice, ctx->stream));
                    if (buf[op.out].lo) WSC_HIP(hipMemcpyAsync((*taps)[k].lo, buf[op.out].lo, nb, hipMemcpyDeviceToDevice, ctx->stream));
                }
    }
    *feat = buf[net->final_buf];
    if (xin_out) *xin_out = xin;
    if (spare) *spare = buf[net->final_buf == 3 ? 2 : 3];
    *hf = pl.hf;
    *wf = pl.wf;
    return WSC_OK;
}

// The classifier branch on the feature map of `count` samples, every `sample_stride`-th of the N in `feat`: global average
// (vgg16) or global max (m7) -> Linear -> Sigmoid.  m7 pools first (layer3_p2, m7_cam.py:32-35).  The maximum of the pooled map
// is the maximum of the map itself unless the pool's windows leave positions out -- a VALID pool whose last window ends before
// the last row or column (9 x 9 under 2 x 2 / 2: row and column 8).  Only then, and only for a `pool_spec` net, the pool is run
// into `spare` and the pooled map reduced; a net without the key keeps the one-pass form whatever the size.
int run_classifier(wsc_ctx *ctx, const wsc_net *net, Act feat, Act spare, int N, int count, int sample_stride, int hf, int wf,
                   float *score_dev) {
    int hw = hf * wf;
    if (net->cls_max && net->cls_pool_set) {
        const PoolSpec &ps = net->cls_pool;
        PoolGeom g;
        WSC_CHECK(pool_geom(ps.rule(), ps.k, ps.stride, 0, false, hf, wf, &g), WSC_ERR_INVALID,
                  "the %d x %d feature map is smaller than the classifier branch's %d x %d VALID pool", hf, wf, ps.k, ps.k);
        const bool crops = !ps.same && ((g.Ho - 1) * ps.stride + ps.k < hf || (g.Wo - 1) * ps.stride + ps.k < wf);
        if (crops) {
            WSC_TRY(launch_pool(ctx, feat, N, hf, wf, net->F, g, spare));
            feat = spare;
            hw = g.Ho * g.Wo;
        }
    }
    return launch_gap_linear_sigmoid(ctx, feat, count, net->cls_max ? -hw : hw, net->F, net->cls_w, net->cls_b, net->Ccls, score_dev,
                                     sample_stride);
}

} // namespace

// GAP / global-max + Linear + Sigmoid, defined in misc_kernels.hip (avg) -- the max flavour
// is selected by a negative hw.
extern "C" {

int wsc_net_create(wsc_ctx *ctx, int arch, const wsc_tensor_desc *weights, int n_weights, int num_classes,
                   int precision, wsc_net **out) {
    WSC_CHECK(ctx && weights && out && n_weights > 0, WSC_ERR_INVALID, "wsc_net_create: null argument");
    WSC_CHECK(num_classes > 0 && num_classes <= 64, WSC_ERR_INVALID, "num_classes=%d outside [1,64]", num_classes);
    wsc_precision prec;
    WSC_TRY(decode_precision(precision, &prec));
    WSC_HIP(hipSetDevice(ctx->device));
    Dict d;
    WSC_TRY(descs_to_dict(weights, n_weights, &d));
    // a checkpoint saved after a diverged step: refused here, in every precision (the maps of such a model are NaN nearly
    // everywhere in the reference)
    for (const auto &kv : d)
        for (int64_t i = 0, n = kv.second.numel(); i < n; ++i)
            WSC_CHECK(std::isfinite(kv.second.data[i]), WSC_ERR_RANGE, "wsc_net_create: state-dict tensor '%s' holds a non-finite value (%g at element %lld)",
                      kv.first.c_str(), (double)kv.second.data[i], (long long)i);
    // (never ignored: the IRN flavours keep the torch port's MaxPool2d(2, 2), the other nets have their own pools)
    WSC_CHECK(!has(d, "pool_spec") || arch == WSC_ARCH_VGG16_CAM || arch == WSC_ARCH_M7_CAM, WSC_ERR_INVALID,
              "pool_spec is a key of WSC_ARCH_VGG16_CAM / WSC_ARCH_M7_CAM only (arch %d)", arch);
    wsc_net *net = new wsc_net();
    net->ctx = ctx;
    net->arch = arch;
    net->C = num_classes;
    net->prec = prec;
    int st;
    switch (arch) {
    case WSC_ARCH_RESNET50_CAM: st = build_resnet50(net, d); break;
    case WSC_ARCH_VGG16_CAM: st = build_vgg16(net, d); break;
    case WSC_ARCH_M7_CAM: st = build_m7(net, d); break;
    case WSC_ARCH_RESNET50_IRN: st = build_resnet50_irn(net, d); break;
    case WSC_ARCH_VGG16_IRN: st = build_vgg16_irn(net, d); break;
    case WSC_ARCH_M7_IRN: st = build_m7_irn(net, d); break;
    case WSC_ARCH_DEEPLAB_LFOV: st = build_deeplab(net, d, false); break;
    case WSC_ARCH_DEEPLAB_ASPP: st = build_deeplab(net, d, true); break;
    default:
        wsc_set_error("unknown arch %d", arch);
        st = WSC_ERR_INVALID;
    }
    if (st != WSC_OK) {
        wsc_net_destroy(net);
        return st;
    }
    *out = net;
    return WSC_OK;
}

void wsc_net_destroy(wsc_net *net) {
    if (!net) return;
    for (void *p : net->allocs) (void)hipFree(p);
    delete net;
}

int wsc_net_cam_size(const wsc_net *net, int S, int *h_out) {
    WSC_CHECK(net && h_out, WSC_ERR_INVALID, "wsc_net_cam_size: null argument");
    Plan pl;
    WSC_TRY(plan_dims(net, 1, S, &pl));
    *h_out = pl.hf;
    return WSC_OK;
}

int wsc_net_feat_channels(const wsc_net *net, int *f_out) {
    WSC_CHECK(net && f_out, WSC_ERR_INVALID, "wsc_net_feat_channels: null argument");
    *f_out = net->F;
    return WSC_OK;
}

int wsc_net_cam_size_hw(const wsc_net *net, int H, int W, int *h_out, int *w_out) {
    WSC_CHECK(net && h_out && w_out, WSC_ERR_INVALID, "wsc_net_cam_size_hw: null argument");
    Plan pl;
    WSC_TRY(plan_dims(net, 1, H, W, &pl));
    *h_out = pl.hf;
    *w_out = pl.wf;
    return WSC_OK;
}

// The 1x1 head (CAM classifier weights / Grad-CAM alpha) with an fp32 NHWC output: in the IEEE-half modes (f16, f16x3) with at
// most 32 classes it is the streaming kernel of cam_head.hip (an HBM stream, not a tile problem); else the tiled kernel.
static int run_head(wsc_ctx *ctx, const ConvLaunch &L) {
    // (K % 256: each wave's quarter of K is whole trips of four 16-channel slices)
    if (conv_fmt(L.prec) == 1 && L.Cout <= 32 && L.CoutPad >= 32 && L.Cin % 256 == 0 && L.y_f32 != nullptr &&
        ctx->opt[WSC_OPT_CAM_HEAD_STREAM] != 0) {
        // (the streaming form checks packing and alignment itself; anything it does not take goes to the tiled kernel)
        WSC_CHECK(L.operands_match(), WSC_ERR_INVALID, "cam head: the input is not of the layer's precision %d", (int)L.prec);
        const int st = launch_cam_head(ctx, L.x, L.N * L.Ho * L.Wo, L.Cin, (const bf16_t *)L.w,
                                       conv_k_layout(L.kh, L.kw, L.Cin, L.form, L.prec).Kw, L.CoutPad, L.s1, L.b1, L.Cout, L.relu, L.y_f32);
        if (st != WSC_ERR_INVALID) return st;
    }
    return conv_igemm_launch(ctx, L);
}

int wsc_net_forward_cam(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int S, float *cam_dev,
                        float *score_dev) {
    return wsc_net_forward_cam_hw(ctx, net, x_dev, B, S, S, cam_dev, score_dev);
}

int wsc_net_forward_cam_hw(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int S, int SW, float *cam_dev,
                           float *score_dev) {
    WSC_CHECK(ctx && net && x_dev && cam_dev, WSC_ERR_INVALID, "wsc_net_forward_cam: null argument");
    WSC_CHECK(B > 0 && S > 0 && SW > 0, WSC_ERR_INVALID, "wsc_net_forward_cam: B=%d input %d x %d", B, S, SW);
    WSC_CHECK(net->head.w != nullptr, WSC_ERR_INVALID, "wsc_net_forward_cam: the network has no CAM head (a segmentation net: wsc_net_forward_seg)");
    WSC_CHECK(score_dev == nullptr || net->cls_w != nullptr, WSC_ERR_INVALID,
              "this architecture has no classifier branch (score_dev must be NULL)");
    WSC_HIP(hipSetDevice(ctx->device));
    const int N = 2 * B;
    Plan pl;
    WSC_TRY(plan_dims(net, N, S, SW, &pl));
    const size_t head_bytes = (size_t)N * pl.hf * pl.wf * net->C * sizeof(float);
    Act feat, spare;
    int hf, wf;
    void *extra;
    WSC_TRY(run_backbone(ctx, net, x_dev, N, S, head_bytes, &feat, &hf, &wf, &extra, nullptr, SW, false, &spare));
    float *head_out = (float *)extra;
    ConvLaunch L = conv_launch(net->head, net->prec);
    L.x = feat;
    L.y_f32 = head_out;
    L.N = N; L.H = hf; L.W = wf; L.Ho = hf; L.Wo = wf;
    WSC_TRY(run_head(ctx, L));
    WSC_TRY(launch_flip_add(ctx, head_out, B, hf, wf, net->C, net->C, cam_dev));
    if (score_dev != nullptr) WSC_TRY(run_classifier(ctx, net, feat, spare, N, B, 2, hf, wf, score_dev));
    return WSC_OK;
}

int wsc_net_forward_gradcam(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, int relu,
                            float *cams_dev, float *score_dev) {
    WSC_CHECK(ctx && net && x_dev && cams_dev, WSC_ERR_INVALID, "wsc_net_forward_gradcam: null argument");
    WSC_CHECK(N > 0 && S > 0, WSC_ERR_INVALID, "wsc_net_forward_gradcam: N=%d S=%d", N, S);
    WSC_CHECK(net->head.w != nullptr, WSC_ERR_INVALID, "wsc_net_forward_gradcam: the network has no CAM head (a segmentation net: wsc_net_forward_seg)");
    WSC_CHECK(score_dev == nullptr || net->cls_w != nullptr, WSC_ERR_INVALID,
              "this architecture has no classifier branch (score_dev must be NULL)");
    WSC_HIP(hipSetDevice(ctx->device));
    Act feat, spare;
    int hf, wf;
    void *extra;
    WSC_TRY(run_backbone(ctx, net, x_dev, N, S, 0, &feat, &hf, &wf, &extra, nullptr, 0, false, &spare));
    ConvLaunch L = conv_launch(net->head, net->prec);
    L.x = feat;
    L.y_f32 = cams_dev; // fp32 NHWC [N][h][w][C]: the layout of np.einsum('ijkl,lm->ijkm')
    L.N = N; L.H = hf; L.W = wf; L.Ho = hf; L.Wo = wf;
    L.relu = relu ? 1 : 0;
    WSC_TRY(run_head(ctx, L));
    if (score_dev != nullptr) WSC_TRY(run_classifier(ctx, net, feat, spare, N, N, 1, hf, wf, score_dev));
    return WSC_OK;
}

int wsc_net_forward_features(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, float *feat_dev) {
    WSC_CHECK(ctx && net && x_dev && feat_dev, WSC_ERR_INVALID, "wsc_net_forward_features: null argument");
    WSC_CHECK(N > 0 && S > 0, WSC_ERR_INVALID, "wsc_net_forward_features: N=%d S=%d", N, S);
    WSC_CHECK(net->seg.empty(), WSC_ERR_INVALID, "wsc_net_forward_features: a segmentation net takes an NHWC input (wsc_net_forward_seg)");
    WSC_HIP(hipSetDevice(ctx->device));
    Act feat;
    int hf, wf;
    void *extra;
    WSC_TRY(run_backbone(ctx, net, x_dev, N, S, 0, &feat, &hf, &wf, &extra));
    return launch_act_to_f32(ctx, feat, (size_t)N * hf * wf * net->F, feat_dev);
}

// ---- the per-op view of a forward pass (tests/test_gpu_net_trace.py) ------------------------------------------------------------
static int trace_plan(const wsc_ctx *ctx, const wsc_net *net, int N, int H, int W, std::vector<wsc_trace_op> *out, Plan *pl) {
    WSC_TRY(plan_dims(net, N, H, W, pl));
    const bool fused = stem_pool_fused(ctx, net);
    int writer[4] = {WSC_TRACE_NONE, WSC_TRACE_NONE, WSC_TRACE_NONE, WSC_TRACE_NONE}; // the op that wrote each rotating buffer last
    auto producer = [&](int b) { return b < 0 ? WSC_TRACE_INPUT : writer[b]; };
    auto set_label = [](wsc_trace_op &t, const std::string &s) {
        std::memset(t.label, 0, sizeof(t.label));
        std::strncpy(t.label, s.c_str(), sizeof(t.label) - 1);
    };
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const Op &op = net->ops[i];
        const OpDims &d = pl->ops[i];
        wsc_trace_op t = {};
        set_label(t, op.label);
        t.in = producer(op.in);
        t.in2 = t.res = WSC_TRACE_NONE;
        t.Ho = d.Ho; t.Wo = d.Wo; t.pitch = d.Co; t.coff = op.coff; t.C = d.Co;
        if (op.type == OP_CONV) {
            const ConvW &c = net->convs[op.conv];
            t.kind = WSC_TRACE_CONV;
            t.C = c.Cout;
            if (op.in2 >= 0) t.in2 = producer(op.in2);
            if (op.res >= 0) t.res = producer(op.res);
            t.kh = c.kh; t.kw = c.kw; t.stride = c.stride; t.pad = c.pad; t.dil = c.dil; t.relu = c.relu;
            t.affine2 = c.s2 != nullptr;
            t.stride2 = op.in2 >= 0 ? op.ps : 0;
            t.fused_next = fused && i == 0;
        } else if (op.type == OP_GATHER) {
            t.kind = WSC_TRACE_GATHER;
            t.C = d.C;
            t.stride = op.ps;
        } else {
            t.kind = WSC_TRACE_POOL;
            t.pool_rule = (int)op.rule; t.pool_k = op.pk; t.pool_stride = op.ps; t.pool_pad = op.pp; t.pool_avg = op.avg;
        }
        writer[op.out] = (int)i;
        out->push_back(t);
    }
    if (net->head.w != nullptr) {
        wsc_trace_op t = {};
        set_label(t, "head");
        t.kind = WSC_TRACE_HEAD;
        t.in = producer(net->final_buf);
        t.in2 = t.res = WSC_TRACE_NONE;
        t.Ho = pl->hf; t.Wo = pl->wf; t.C = t.pitch = net->C;
        t.kh = t.kw = t.stride = t.dil = 1;
        out->push_back(t);
    }
    return WSC_OK;
}

int wsc_net_trace_plan(wsc_ctx *ctx, const wsc_net *net, int N, int H, int W, wsc_trace_op *ops_out, int max_ops, int *n_ops_out) {
    WSC_CHECK(ctx && net && n_ops_out, WSC_ERR_INVALID, "wsc_net_trace_plan: null argument");
    WSC_CHECK(N > 0 && H > 0 && W > 0 && max_ops >= 0 && (ops_out != nullptr || max_ops == 0), WSC_ERR_INVALID,
              "wsc_net_trace_plan: N=%d input %d x %d, room for %d ops", N, H, W, max_ops);
    std::vector<wsc_trace_op> ops;
    Plan pl;
    WSC_TRY(trace_plan(ctx, net, N, H, W, &ops, &pl));
    *n_ops_out = (int)ops.size();
    for (int i = 0; i < max_ops && i < (int)ops.size(); ++i) ops_out[i] = ops[i];
    return WSC_OK;
}

int wsc_net_forward_trace(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int H, int W, const long long *offsets_host,
                          int n_offsets, float *trace_dev, long long trace_elems) {
    WSC_CHECK(ctx && net && x_dev && offsets_host && trace_dev, WSC_ERR_INVALID, "wsc_net_forward_trace: null argument");
    WSC_CHECK(N > 0 && H > 0 && W > 0 && trace_elems >= 0, WSC_ERR_INVALID, "wsc_net_forward_trace: N=%d input %d x %d", N, H, W);
    WSC_HIP(hipSetDevice(ctx->device));
    std::vector<wsc_trace_op> ops;
    Plan pl;
    WSC_TRY(trace_plan(ctx, net, N, H, W, &ops, &pl));
    WSC_CHECK(n_offsets == (int)ops.size(), WSC_ERR_INVALID, "wsc_net_forward_trace: %d offsets for %d entries (wsc_net_trace_plan)", n_offsets,
              (int)ops.size());
    // every wanted entry lies inside the caller's buffer, and is an op this run computes on its own
    for (int i = 0; i < n_offsets; ++i) {
        if (offsets_host[i] < 0) continue;
        const long long elems = (long long)N * ops[i].Ho * ops[i].Wo * ops[i].pitch;
        WSC_CHECK(!ops[i].fused_next, WSC_ERR_INVALID, "wsc_net_forward_trace: op %d is computed together with op %d in this run", i, i + 1);
        WSC_CHECK(offsets_host[i] <= trace_elems - elems, WSC_ERR_INVALID, "wsc_net_forward_trace: entry %d (%lld floats at %lld) leaves the %lld-float buffer",
                  i, elems, offsets_host[i], trace_elems);
    }
    const bool has_head = net->head.w != nullptr;
    const size_t head_bytes = has_head ? (size_t)N * pl.hf * pl.wf * net->C * sizeof(float) : 0;
    const TraceSink sink = {offsets_host, trace_dev};
    Act feat, spare;
    int hf, wf;
    void *extra;
    WSC_TRY(run_backbone(ctx, net, x_dev, N, H, head_bytes, &feat, &hf, &wf, &extra, nullptr, W, !net->seg.empty(), &spare, &sink));
    if (has_head && offsets_host[n_offsets - 1] >= 0) {
        float *head_out = (float *)extra; // (as wsc_net_forward_cam_hw has it, before the flip-add)
        ConvLaunch L = conv_launch(net->head, net->prec);
        L.x = feat;
        L.y_f32 = head_out;
        L.N = N; L.H = hf; L.W = wf; L.Ho = hf; L.Wo = wf;
        WSC_TRY(run_head(ctx, L));
        WSC_HIP(hipMemcpyAsync(trace_dev + offsets_host[n_offsets - 1], head_out, head_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return WSC_OK;
}

// Net.forward (resnet50_irn.py:110-133 / vgg16_irn.py:192-212) for N samples [N][3][S][S], the body wsc_net_forward_edge and
// wsc_net_forward_edge_raw share: backbone with stage taps -> 12 Conv-GroupNorm-[Upsample]-ReLU heads into three concat
// buffers -> fc_edge6 / fc_dp7[3].  The two maps stay in the workspace: e [N][He][We], d [N][Hd][Wd][2].
struct EdgeMaps {
    float *e, *d;
    int He, We, Hd, Wd;
};
// The sizes of everything between the stage taps and the two maps for N samples of S x S
struct EdgeGeom {
    Plan pl;
    std::vector<int> Hs, Ws, Cs;             // stage taps
    std::vector<int> cat_c, cat_h, cat_w;    // concat buffers
    std::vector<size_t> cat_elems;
    struct Head { int sh, sw, sc, ho, wo; }; // a head's source tensor and its conv output (before the upsample)
    std::vector<Head> heads;
    int He, We, Hd, Wd;
};
static int edge_outdim(int v, int stride) { return (v - 1) / stride + 1; }
static int edge_geom(const wsc_net *net, int N, int S, EdgeGeom *g) {
    WSC_TRY(plan_dims(net, N, S, &g->pl));
    const int NS = (int)net->taps.size(), NC = (int)net->cats.size();
    g->Hs.resize(NS); g->Ws.resize(NS); g->Cs.resize(NS);
    for (int k = 0; k < NS; ++k) {
        const OpDims &d = g->pl.ops[net->taps[k]];
        g->Hs[k] = d.Ho; g->Ws[k] = d.Wo; g->Cs[k] = d.Co;
    }
    g->cat_c.resize(NC); g->cat_h.resize(NC); g->cat_w.resize(NC); g->cat_elems.resize(NC);
    for (int i = 0; i < NC; ++i) {
        const IrnCat &c = net->cats[i];
        g->cat_c[i] = c.channels;
        g->cat_h[i] = edge_outdim(g->Hs[c.stage - 1], c.stride);
        g->cat_w[i] = edge_outdim(g->Ws[c.stage - 1], c.stride);
        g->cat_elems[i] = (size_t)N * g->cat_h[i] * g->cat_w[i] * g->cat_c[i];
    }
    g->He = g->cat_h[0]; g->We = g->cat_w[0]; g->Hd = g->cat_h[NC - 1]; g->Wd = g->cat_w[NC - 1]; // edge / displacement maps
    g->heads.clear();
    for (const IrnHead &h : net->heads) {
        const int k = h.src > 0 ? h.src - 1 : -h.src - 1; // a stage tap, or a concat buffer
        EdgeGeom::Head hg;
        hg.sh = h.src > 0 ? g->Hs[k] : g->cat_h[k];
        hg.sw = h.src > 0 ? g->Ws[k] : g->cat_w[k];
        hg.sc = h.src > 0 ? g->Cs[k] : g->cat_c[k];
        hg.ho = edge_outdim(hg.sh, h.conv.stride);
        hg.wo = edge_outdim(hg.sw, h.conv.stride);
        g->heads.push_back(hg);
    }
    return WSC_OK;
}

// The layout of a tape: float32 tensors [N][Ho][Wo][C] in one buffer of `elems` floats, each on a 256-byte line.  Every training
// path's tape plan embeds this one and keeps only its own indices into `e` (embed it, do not copy it).
struct TapeLayout {
    std::vector<wsc_tape_entry> e;
    long long elems = 0;
    int add(const std::string &name, int N, int Ho, int Wo, int C) {
        wsc_tape_entry t = {};
        std::strncpy(t.name, name.c_str(), sizeof(t.name) - 1);
        t.Ho = Ho; t.Wo = Wo; t.C = C;
        t.offset = elems;
        elems += ((long long)N * Ho * Wo * C + 63) / 64 * 64; // (entries start on 256-byte lines)
        e.push_back(t);
        return (int)e.size() - 1;
    }
    long long off(int entry) const { return e[entry].offset; }
};
// the out-parameters of a wsc_net_*_tape_plan entry (entries_out may be short or null: n_out is the whole count)
static int tape_export(const TapeLayout &t, wsc_tape_entry *entries_out, int max_entries, int *n_out, long long *tape_elems_out) {
    *n_out = (int)t.e.size();
    *tape_elems_out = t.elems;
    for (int i = 0; i < max_entries && i < (int)t.e.size(); ++i) entries_out[i] = t.e[i];
    return WSC_OK;
}
// the caller's tape is the one `plan_fn` describes, checked before anything is launched
static int tape_check(const char *fn, const char *plan_fn, long long tape_elems, const TapeLayout &t) {
    WSC_CHECK(tape_elems == t.elems, WSC_ERR_INVALID, "%s: a tape of %lld floats, the plan has %lld (%s)", fn, tape_elems, t.elems, plan_fn);
    return WSC_OK;
}

// one guard per net kind, under the name of the entry point that asks
static int need_irn(const char *fn, const wsc_net *net) {
    WSC_CHECK(!net->heads.empty() && net->cats.size() >= 2, WSC_ERR_INVALID, "%s: the network is not an IRNet EdgeDisplacement net", fn);
    return WSC_OK;
}
static int need_seg(const char *fn, const wsc_net *net) {
    WSC_CHECK(!net->seg.empty(), WSC_ERR_INVALID, "%s: the network is not a WSC_ARCH_DEEPLAB_* net", fn);
    return WSC_OK;
}

// What the backward pass of the heads needs of a forward pass, as float32 in one buffer (each "the value the next op read": hi +
// lo of a two-plane precision): every stage tap a head reads "x<k>" [N][H][W][C]; per head its conv output "<head>.z"
// [N][ho][wo][Cout] and its GroupNorm statistics "<head>.stats" [N][1][1][2 G] = {mean, rstd} pairs as gn_finish_kernel wrote
// them; every concat buffer "cat<i>" [N][Hc][Wc][Ctot], padding channels included
struct EdgeTapePlan {
    EdgeGeom g;
    TapeLayout t;
    std::vector<int> tap, z, stats, cat; // entry of stage k (-1: no head reads it), of head j (two), of concat buffer i
};
static int edge_tape_plan(const wsc_net *net, int N, int S, EdgeTapePlan *tp) {
    WSC_TRY(edge_geom(net, N, S, &tp->g));
    const EdgeGeom &g = tp->g;
    auto add = [&](const std::string &name, int Ho, int Wo, int C) { return tp->t.add(name, N, Ho, Wo, C); };
    tp->tap.assign(net->taps.size(), -1);
    for (size_t k = 0; k < net->taps.size(); ++k) {
        bool read = false;
        for (const IrnHead &h : net->heads) read = read || h.src == (int)k + 1;
        if (read) tp->tap[k] = add("x" + std::to_string(k + 1), g.Hs[k], g.Ws[k], g.Cs[k]);
    }
    for (size_t j = 0; j < net->heads.size(); ++j) {
        const IrnHead &h = net->heads[j];
        tp->z.push_back(add(h.name + ".z", g.heads[j].ho, g.heads[j].wo, h.conv.Cout));
        tp->stats.push_back(add(h.name + ".stats", 1, 1, 2 * h.groups));
    }
    for (size_t i = 0; i < net->cats.size(); ++i) tp->cat.push_back(add("cat" + std::to_string(i), g.cat_h[i], g.cat_w[i], g.cat_c[i]));
    return WSC_OK;
}

// feat_h > 0: the crop (feat_h, feat_w) is checked against the maps before anything runs; x_dev == nullptr: the sizes alone.
// tp / tape (wsc_net_forward_edge_tape): the same launches; a head's conv and statistics kernels write straight into their tape
// entries (instead of the scratch they otherwise use), the taps and the concat buffers are copied
static int forward_edge_maps(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, int feat_h, int feat_w, EdgeMaps *out,
                             const EdgeTapePlan *tp = nullptr, float *tape = nullptr) {
    EdgeGeom geom;
    if (!tp) WSC_TRY(edge_geom(net, N, S, &geom));
    const EdgeGeom &g = tp ? tp->g : geom;
    const Plan &pl = g.pl;
    const int NC = (int)net->cats.size();
    const std::vector<int> &Hs = g.Hs, &Ws = g.Ws, &Cs = g.Cs, &cat_c = g.cat_c, &cat_h = g.cat_h, &cat_w = g.cat_w;
    const std::vector<size_t> &cat_elems = g.cat_elems;
    size_t off = taps_bytes(net, pl, N); // workspace after the backbone's: taps, concat buffers, then the scratch below
    for (int i = 0; i < NC; ++i) off += act_bytes(cat_elems[i], net->prec);
    const int He = g.He, We = g.We, Hd = g.Hd, Wd = g.Wd;
    WSC_CHECK(feat_h <= He && feat_w <= We && feat_h <= Hd && feat_w <= Wd, WSC_ERR_INVALID,
              "feature size %dx%d exceeds the head resolution %dx%d / %dx%d", feat_h, feat_w, He, We, Hd, Wd);
    out->e = out->d = nullptr;
    out->He = He; out->We = We; out->Hd = Hd; out->Wd = Wd;
    if (!x_dev) return WSC_OK;
    size_t ftmp_elems = 0, part_bytes = 0;
    int max_groups = 1;
    for (size_t j = 0; j < net->heads.size(); ++j) {
        const IrnHead &h = net->heads[j];
        const int ho = g.heads[j].ho, wo = g.heads[j].wo;
        ftmp_elems = std::max(ftmp_elems, (size_t)N * ho * wo * h.conv.Cout);
        part_bytes = std::max(part_bytes, group_norm_partial_bytes(N, ho, wo, h.groups));
        max_groups = std::max(max_groups, h.groups);
    }
    // head conv output, GroupNorm partial sums, GroupNorm statistics, edge map, displacement map
    const size_t scratch[5] = {ftmp_elems * sizeof(float), part_bytes, sizeof(float) * 2 * N * max_groups,
                               sizeof(float) * (size_t)N * He * We, sizeof(float) * (size_t)N * Hd * Wd * 2};
    for (size_t b : scratch) off += align_up(b, 256);

    Act feat;
    int hf, wf;
    void *extra;
    std::vector<Act> taps, cats;
    WSC_TRY(run_backbone(ctx, net, x_dev, N, S, off, &feat, &hf, &wf, &extra, &taps));
    char *p = (char *)extra;
    for (int i = 0; i < NC; ++i) cats.push_back(act_carve(p, cat_elems[i], net->prec));
    char *sp[5];
    for (int i = 0; i < 5; ++i) { sp[i] = p; p += align_up(scratch[i], 256); }
    float *ftmp = (float *)sp[0], *e_out = (float *)sp[3], *d_out = (float *)sp[4];
    void *gn_part = sp[1], *gn_stats = sp[2];
    // the padding channels of the edge concat feed zero weights but must not hold NaN bit patterns
    WSC_HIP(hipMemsetAsync(cats[0].hi, 0, act_bytes(cat_elems[0], net->prec), ctx->stream));
    if (tp)
        for (size_t k = 0; k < taps.size(); ++k)
            if (tp->tap[k] >= 0) WSC_TRY(launch_act_to_f32(ctx, taps[k], (size_t)N * Hs[k] * Ws[k] * Cs[k], tape + tp->t.off(tp->tap[k])));

    auto run_conv = [&](const ConvW &c, Act x, int H, int W, float *y_f32) -> int {
        ConvLaunch L = conv_launch(c, net->prec); // (1 x 1, no padding, no ReLU: build_irn_heads)
        L.x = x;
        L.y_f32 = y_f32;
        L.N = N; L.H = H; L.W = W; L.Ho = edge_outdim(H, c.stride); L.Wo = edge_outdim(W, c.stride);
        return conv_igemm_launch(ctx, L);
    };
    for (size_t j = 0; j < net->heads.size(); ++j) {
        const IrnHead &h = net->heads[j];
        const EdgeGeom::Head &hg = g.heads[j];
        const int k = h.src > 0 ? h.src - 1 : -h.src - 1; // a stage tap, or a concat buffer
        const Act x = h.src > 0 ? taps[k] : cats[k];
        WSC_CHECK(hg.sc == h.conv.Cin, WSC_ERR_SHAPE, "IRNet head: %d input channels, the weights expect %d", hg.sc, h.conv.Cin);
        float *z = tp ? tape + tp->t.off(tp->z[j]) : ftmp;
        void *stats = tp ? (void *)(tape + tp->t.off(tp->stats[j])) : gn_stats;
        WSC_TRY(run_conv(h.conv, x, hg.sh, hg.sw, z));
        WSC_TRY(launch_group_norm_stats(ctx, z, N, hg.ho, hg.wo, h.conv.Cout, h.groups, 1e-5f, gn_part, stats));
        const int di = h.dst;
        WSC_TRY(launch_group_norm_apply(ctx, z, stats, h.gamma, h.beta, N, hg.ho, hg.wo, h.conv.Cout, h.groups,
                                        h.up, 1, cats[di], cat_h[di], cat_w[di], cat_c[di], h.coff));
    }
    if (tp)
        for (int i = 0; i < NC; ++i) WSC_TRY(launch_act_to_f32(ctx, cats[i], cat_elems[i], tape + tp->t.off(tp->cat[i])));
    WSC_TRY(run_conv(net->edge6, cats[0], He, We, e_out));
    WSC_TRY(run_conv(net->dp7b, cats[NC - 1], Hd, Wd, d_out));
    out->e = e_out;
    out->d = d_out;
    return WSC_OK;
}

// EdgeDisplacement.forward (resnet50_irn.py:212-232 / vgg16_irn.py:306-321) for B images: x is the
// [orig, h-flip] pair of each image already zero-padded to the crop size S (F.pad(x, [0, S-w, 0, S-h])).
// Net.forward -> crop to (feat_h, feat_w), sigmoid(edge[0]/2 + edge[1].flip(-1)/2), dp[0] - mean_shift.
int wsc_net_forward_edge(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int S, int feat_h, int feat_w,
                         float *edge_dev, float *dp_dev) {
    WSC_CHECK(ctx && net && x_dev && edge_dev && dp_dev, WSC_ERR_INVALID, "wsc_net_forward_edge: null argument");
    WSC_TRY(need_irn("wsc_net_forward_edge", net));
    WSC_CHECK(B > 0 && S > 0 && feat_h > 0 && feat_w > 0, WSC_ERR_INVALID, "wsc_net_forward_edge: B=%d S=%d", B, S);
    WSC_HIP(hipSetDevice(ctx->device));
    EdgeMaps m;
    WSC_TRY(forward_edge_maps(ctx, net, x_dev, 2 * B, S, feat_h, feat_w, &m));
    WSC_TRY(launch_edge_finish(ctx, m.e, m.He, m.We, m.d, m.Hd, m.Wd, B, feat_h, feat_w, net->mean_shift[0],
                               net->mean_shift[1], edge_dev, dp_dev));
    return WSC_OK;
}

// (He, We) and (Hd, Wd) of the two maps for an S x S input
int wsc_net_edge_size(const wsc_net *net, int S, int *edge_hw, int *dp_hw) {
    WSC_CHECK(net && edge_hw && dp_hw, WSC_ERR_INVALID, "wsc_net_edge_size: null argument");
    WSC_TRY(need_irn("wsc_net_edge_size", net));
    WSC_CHECK(S > 0, WSC_ERR_INVALID, "wsc_net_edge_size: S=%d", S);
    EdgeMaps m;
    WSC_TRY(forward_edge_maps(nullptr, net, nullptr, 1, S, 0, 0, &m));
    edge_hw[0] = m.He; edge_hw[1] = m.We;
    dp_hw[0] = m.Hd; dp_hw[1] = m.Wd;
    return WSC_OK;
}

// Net.forward in training mode (resnet50_irn.py:110-133): N plain samples, no flip pairing, no crop, MeanShift the identity, no sigmoid
int wsc_net_forward_edge_raw(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, float *edge_dev, float *dp_dev) {
    WSC_CHECK(ctx && net && x_dev && edge_dev && dp_dev, WSC_ERR_INVALID, "wsc_net_forward_edge_raw: null argument");
    WSC_TRY(need_irn("wsc_net_forward_edge_raw", net));
    WSC_CHECK(N > 0 && S > 0, WSC_ERR_INVALID, "wsc_net_forward_edge_raw: N=%d S=%d", N, S);
    WSC_HIP(hipSetDevice(ctx->device));
    EdgeMaps m;
    WSC_TRY(forward_edge_maps(ctx, net, x_dev, N, S, 0, 0, &m));
    return launch_edge_raw(ctx, m.e, m.He, m.We, m.d, m.Hd, m.Wd, N, edge_dev, dp_dev);
}

int wsc_net_edge_tape_plan(wsc_ctx *ctx, const wsc_net *net, int N, int S, wsc_tape_entry *entries_out, int max_entries, int *n_out,
                           long long *tape_elems_out) {
    WSC_CHECK(ctx && net && n_out && tape_elems_out, WSC_ERR_INVALID, "wsc_net_edge_tape_plan: null argument");
    WSC_TRY(need_irn("wsc_net_edge_tape_plan", net));
    WSC_CHECK(N > 0 && S > 0 && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_net_edge_tape_plan: N=%d S=%d, room for %d entries", N, S, max_entries);
    EdgeTapePlan tp;
    WSC_TRY(edge_tape_plan(net, N, S, &tp));
    return tape_export(tp.t, entries_out, max_entries, n_out, tape_elems_out);
}

int wsc_net_forward_edge_tape(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, float *tape_dev, long long tape_elems,
                              float *edge_dev, float *dp_dev) {
    WSC_CHECK(ctx && net && x_dev && tape_dev && edge_dev && dp_dev, WSC_ERR_INVALID, "wsc_net_forward_edge_tape: null argument");
    WSC_TRY(need_irn("wsc_net_forward_edge_tape", net));
    WSC_CHECK(N > 0 && S > 0, WSC_ERR_INVALID, "wsc_net_forward_edge_tape: N=%d S=%d", N, S);
    WSC_CHECK(((uintptr_t)tape_dev & 255) == 0, WSC_ERR_INVALID, "wsc_net_forward_edge_tape: the tape must start on a 256-byte line");
    EdgeTapePlan tp;
    WSC_TRY(edge_tape_plan(net, N, S, &tp));
    WSC_TRY(tape_check("wsc_net_forward_edge_tape", "wsc_net_edge_tape_plan", tape_elems, tp.t));
    WSC_HIP(hipSetDevice(ctx->device));
    EdgeMaps m;
    WSC_TRY(forward_edge_maps(ctx, net, x_dev, N, S, 0, 0, &m, &tp, tape_dev));
    return launch_edge_raw(ctx, m.e, m.He, m.We, m.d, m.Hd, m.Wd, N, edge_dev, dp_dev);
}

// The DeepLab forward pass of SEC / DSRG (create_network up to "fc8-softmax", SEC.py:117-128,246-249 / DSRG.py:169-186,297-300)
int wsc_net_seg_size_hw(const wsc_net *net, int H, int W, int *h_out, int *w_out) {
    WSC_CHECK(net && h_out && w_out, WSC_ERR_INVALID, "wsc_net_seg_size_hw: null argument");
    WSC_TRY(need_seg("wsc_net_seg_size_hw", net));
    WSC_CHECK(H >= 1 && W >= 1, WSC_ERR_INVALID, "wsc_net_seg_size_hw: input %d x %d", H, W);
    Plan pl;
    WSC_TRY(plan_dims(net, 1, H, W, &pl));
    *h_out = pl.hf;
    *w_out = pl.wf;
    return WSC_OK;
}

// The tensors a backward pass needs of a forward pass ("the tape"), as float32 NHWC in one buffer: the network input, every op's
// output of the trunk (the last pool is pool5a), every branch's fc6 and fc7 -- each the value the next op read (hi + lo)
struct TapePlan {
    Plan pl;
    TapeLayout t;
    std::vector<int> op_entry;   // entry of op i's output
    std::vector<int> fc6, fc7;   // entries of branch k
};
static int seg_tape_plan(const wsc_net *net, int B, int H, int W, TapePlan *tp) {
    WSC_TRY(plan_dims(net, B, H, W, &tp->pl));
    auto add = [&](const std::string &name, int Ho, int Wo, int C) { return tp->t.add(name, B, Ho, Wo, C); };
    add("input", H, W, 3);
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const Op &op = net->ops[i];
        const OpDims &d = tp->pl.ops[i];
        // (the backward pass walks a chain: every op reads the op before it and nothing else)
        WSC_CHECK(op.type != OP_GATHER && op.res < 0 && op.in2 < 0 && op.pitch == 0 && (i == 0 ? op.in < 0 : op.in == net->ops[i - 1].out),
                  WSC_ERR_INVALID, "internal: op %d of a segmentation net is no link of a chain", (int)i);
        tp->op_entry.push_back(add(i + 1 == net->ops.size() && op.type == OP_POOL && op.avg ? "pool5a" : op.label, d.Ho, d.Wo, d.Co));
    }
    for (size_t k = 0; k < net->seg.size(); ++k) {
        const std::string sfx = net->seg.size() > 1 ? "_" + std::to_string(k + 1) : "";
        tp->fc6.push_back(add("fc6" + sfx, tp->pl.hf, tp->pl.wf, net->seg[k].fc6.Cout));
        tp->fc7.push_back(add("fc7" + sfx, tp->pl.hf, tp->pl.wf, net->seg[k].fc7.Cout));
    }
    return WSC_OK;
}

// the dropout sites of a training forward pass (wsc_net_forward_seg_train); drop_prob = 0: none, the launches of the tape pass
struct SegDropout {
    float drop_prob = 0.f;
    unsigned long long seed = 0;
    unsigned step = 0;
};
// wsc_net_forward_seg (tp null) and wsc_net_forward_seg_tape: the same launches; with a tape, copies between them.  drop (with a
// tape, drop_prob > 0): the copy behind fc6 / fc7 of branch k is the dropout kernel of site 2 k / 2 k + 1 instead, which drops
// and scales the activation in place and writes the tape entry in the same pass.
static int forward_seg(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob, float *fc8_dev,
                       float *prob_dev, const TapePlan *tp, float *tape, const SegDropout *drop = nullptr) {
    Plan pl;
    WSC_TRY(plan_dims(net, B, H, W, &pl));
    const size_t M = (size_t)B * pl.hf * pl.wf;
    // behind the trunk's buffers: fc6's and fc7's outputs (one pair, the branches run one after the other), then every
    // branch's fp32 logits -- kept at fp32 and summed by the softmax kernel in the reference's order fc8_1 + fc8_2 + fc8_3 + fc8_4
    size_t e6 = 0, e7 = 0;
    for (const SegBranch &br : net->seg) {
        e6 = std::max(e6, M * br.fc6.Cout);
        e7 = std::max(e7, M * br.fc7.Cout);
    }
    const size_t logit_bytes = align_up(M * net->C * sizeof(float), 256);
    // (tape: behind those, the NHWC4 input as fp32 on its way to the tape's 3-channel entry)
    const size_t in4_elems = (size_t)B * H * W * 4;
    const size_t extra_bytes = act_bytes(e6, net->prec) + act_bytes(e7, net->prec) + net->seg.size() * logit_bytes +
                               (tp ? in4_elems * sizeof(float) : 0);
    Act feat, xin;
    int hf, wf;
    void *extra;
    std::vector<long long> op_off;
    if (tp)
        for (int e : tp->op_entry) op_off.push_back(tp->t.off(e));
    const TraceSink sink = {op_off.data(), tape};
    WSC_TRY(run_backbone(ctx, net, x_dev, B, H, extra_bytes, &feat, &hf, &wf, &extra, nullptr, W, true, nullptr, tp ? &sink : nullptr, &xin));
    char *p = (char *)extra;
    if (tp) {
        float *in4 = (float *)(p + extra_bytes - in4_elems * sizeof(float));
        WSC_TRY(launch_act_to_f32(ctx, xin, in4_elems, in4));
        WSC_TRY(launch_copy_channels(ctx, in4, (long long)B * H * W, 4, 3, tape + tp->t.off(0)));
    }
    const Act a6 = act_carve(p, e6, net->prec), a7 = act_carve(p, e7, net->prec);
    const float *logits[4] = {nullptr, nullptr, nullptr, nullptr};
    WSC_CHECK(net->seg.size() <= 4, WSC_ERR_INVALID, "internal: %d head branches", (int)net->seg.size());
    for (size_t k = 0; k < net->seg.size(); ++k) {
        const SegBranch &br = net->seg[k];
        float *out = (float *)(p + k * logit_bytes);
        logits[k] = out;
        auto run = [&](const ConvW &c, Act x, Act y, float *y_f32) -> int {
            ConvLaunch L = conv_launch(c, net->prec);
            L.x = x; L.y = y; L.y_f32 = y_f32;
            L.N = B; L.H = hf; L.W = wf; L.Ho = hf; L.Wo = wf; // (SAME at stride 1: pad = dil (k - 1) / 2)
            return conv_igemm_launch(ctx, L);
        };
        const bool dropping = tp && drop && drop->drop_prob > 0.f;
        auto keep = [&](Act a, int Cout, int entry, unsigned site) -> int {
            if (!tp) return WSC_OK;
            float *dst = tape + tp->t.off(entry);
            if (dropping) return launch_seg_dropout(ctx, a, M * Cout, Cout, drop->drop_prob, drop->seed, drop->step, site, dst);
            return launch_act_to_f32(ctx, a, M * Cout, dst);
        };
        WSC_TRY(run(br.fc6, feat, a6, nullptr));
        WSC_TRY(keep(a6, br.fc6.Cout, tp ? tp->fc6[k] : 0, 2u * (unsigned)k));
        WSC_TRY(run(br.fc7, a6, a7, nullptr));
        WSC_TRY(keep(a7, br.fc7.Cout, tp ? tp->fc7[k] : 0, 2u * (unsigned)k + 1u));
        WSC_TRY(run(br.fc8, a7, Act(), out));
    }
    return launch_fc8_softmax(ctx, logits, (int)net->seg.size(), (long long)M, net->C, min_prob, fc8_dev, prob_dev);
}

int wsc_net_forward_seg(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob, float *fc8_dev,
                        float *prob_dev) {
    WSC_CHECK(ctx && net && x_dev && prob_dev, WSC_ERR_INVALID, "wsc_net_forward_seg: null argument");
    WSC_TRY(need_seg("wsc_net_forward_seg", net));
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1 && min_prob >= 0.f, WSC_ERR_INVALID, "wsc_net_forward_seg: B=%d input %d x %d min_prob=%g", B, H, W,
              (double)min_prob);
    WSC_HIP(hipSetDevice(ctx->device));
    return forward_seg(ctx, net, x_dev, B, H, W, min_prob, fc8_dev, prob_dev, nullptr, nullptr);
}

int wsc_net_seg_tape_plan(wsc_ctx *ctx, const wsc_net *net, int B, int H, int W, wsc_tape_entry *entries_out, int max_entries, int *n_out,
                          long long *tape_elems_out) {
    WSC_CHECK(ctx && net && n_out && tape_elems_out, WSC_ERR_INVALID, "wsc_net_seg_tape_plan: null argument");
    WSC_TRY(need_seg("wsc_net_seg_tape_plan", net));
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1 && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_net_seg_tape_plan: B=%d input %d x %d, room for %d entries", B, H, W, max_entries);
    TapePlan tp;
    WSC_TRY(seg_tape_plan(net, B, H, W, &tp));
    return tape_export(tp.t, entries_out, max_entries, n_out, tape_elems_out);
}

int wsc_net_forward_seg_tape(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob, float *tape_dev,
                             long long tape_elems, float *fc8_dev, float *prob_dev) {
    WSC_CHECK(ctx && net && x_dev && prob_dev && tape_dev, WSC_ERR_INVALID, "wsc_net_forward_seg_tape: null argument");
    WSC_TRY(need_seg("wsc_net_forward_seg_tape", net));
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1 && min_prob >= 0.f, WSC_ERR_INVALID, "wsc_net_forward_seg_tape: B=%d input %d x %d min_prob=%g", B, H,
              W, (double)min_prob);
    TapePlan tp;
    WSC_TRY(seg_tape_plan(net, B, H, W, &tp));
    WSC_TRY(tape_check("wsc_net_forward_seg_tape", "wsc_net_seg_tape_plan", tape_elems, tp.t));
    WSC_HIP(hipSetDevice(ctx->device));
    return forward_seg(ctx, net, x_dev, B, H, W, min_prob, fc8_dev, prob_dev, &tp, tape_dev);
}

int wsc_net_forward_seg_train(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob, float drop_prob,
                              unsigned long long seed, long long step, float *tape_dev, long long tape_elems, float *fc8_dev,
                              float *prob_dev) {
    WSC_CHECK(ctx && net && x_dev && prob_dev && tape_dev, WSC_ERR_INVALID, "wsc_net_forward_seg_train: null argument");
    WSC_TRY(need_seg("wsc_net_forward_seg_train", net));
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1 && min_prob >= 0.f, WSC_ERR_INVALID, "wsc_net_forward_seg_train: B=%d input %d x %d min_prob=%g", B, H,
              W, (double)min_prob);
    WSC_TRY(seg_dropout_check("wsc_net_forward_seg_train", drop_prob, step));
    TapePlan tp;
    WSC_TRY(seg_tape_plan(net, B, H, W, &tp));
    WSC_TRY(tape_check("wsc_net_forward_seg_train", "wsc_net_seg_tape_plan", tape_elems, tp.t));
    WSC_HIP(hipSetDevice(ctx->device));
    SegDropout drop;
    drop.drop_prob = drop_prob; drop.seed = seed; drop.step = (unsigned)step;
    return forward_seg(ctx, net, x_dev, B, H, W, min_prob, fc8_dev, prob_dev, &tp, tape_dev, &drop);
}

// ---- the backward pass of the DeepLab nets: d loss / d fc8 -> the gradient of every weight and bias -----------------------------
namespace {
// What the gradient object of every training path owns: the context and the net it was made for, its device allocations, the ones
// and zeros of the data-gradient GEMM, the backward workspace, the repack jobs of its load-params entry, the size of its flat
// layout.  wsc_seg_grad, wsc_irn_grad and wsc_cls_grad derive from it and keep only what differs (embed it, do not
// copy it).
struct GradCore {
    const char *kind; // the C type's name, for the messages
    wsc_ctx *ctx;
    const wsc_net *net;
    long long grad_elems = 0;
    float *ones = nullptr, *zeros = nullptr; // conv_cout_pad(widest input of a data-gradient GEMM) of each
    void *ws = nullptr;                      // the backward workspace, grown on demand
    size_t ws_bytes = 0;
    RepackPlan repack;                       // the jobs of the load-params entry, built by its first call
    std::vector<void *> allocs;
    GradCore(const char *kind_, wsc_ctx *ctx_, const wsc_net *net_) : kind(kind_), ctx(ctx_), net(net_) {}

    int own(size_t bytes, void **dst) {
        WSC_HIP(hipMalloc(dst, bytes));
        allocs.push_back(*dst);
        return WSC_OK;
    }
    int zeroed(size_t bytes, void **dst) {
        WSC_TRY(own(bytes, dst));
        WSC_HIP(hipMemset(*dst, 0, bytes));
        return WSC_OK;
    }
    int upload(const void *host, size_t bytes, void **dst) {
        WSC_TRY(own(bytes, dst));
        WSC_HIP(hipMemcpy(*dst, host, bytes, hipMemcpyHostToDevice));
        return WSC_OK;
    }
    int upload(const std::vector<float> &v, float **dst) { return upload(v.data(), v.size() * sizeof(float), (void **)dst); }
    // `widest` ones and as many zeros
    int ones_zeros(int widest) {
        WSC_TRY(upload(std::vector<float>(widest, 1.f), &ones));
        return upload(std::vector<float>(widest, 0.f), &zeros);
    }
    // at least `need` bytes of workspace on the object's stream, wsc_ctx_scratch_fill applied: the workspace is scratch like the
    // arena -- nothing in it outlives a call
    int workspace(size_t need) {
        WSC_HIP(hipSetDevice(ctx->device));
        if (need > ws_bytes) {
            if (ws) {
                WSC_HIP(hipStreamSynchronize(ctx->stream));
                WSC_HIP(hipFree(ws));
                ws = nullptr;
                ws_bytes = 0;
            }
            WSC_HIP(hipMalloc(&ws, need));
            ws_bytes = need;
        }
        if (ctx->scratch_fill >= 0) WSC_HIP(hipMemsetAsync(ws, ctx->scratch_fill, ws_bytes, ctx->stream));
        return WSC_OK;
    }
    // the job table of the load-params entry and the scratch of its channel maxima, once per object (the packed buffers never move)
    // (dst: another plan of the object than `repack`)
    int plan_repack(std::vector<RepackJob> &jobs, RepackPlan *dst = nullptr) {
        RepackPlan plan;
        void *jd = nullptr, *pm = nullptr;
        WSC_TRY(repack_plan(jobs, net->prec, &plan));
        WSC_TRY(upload(jobs.data(), jobs.size() * sizeof(RepackJob), &jd));
        if (plan.pmax_elems > 0) WSC_TRY(own((size_t)plan.pmax_elems * sizeof(float), &pm));
        plan.pmax = (float *)pm;
        plan.jobs_dev = (RepackJob *)jd;
        *(dst ? dst : &repack) = plan;
        return WSC_OK;
    }
    void release() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : allocs) (void)hipFree(p);
        if (ws) (void)hipFree(ws);
    }
};
// A device table of jobs that each carry `block0`, their first block in one launch: add() hands a job its blocks, jobs in order,
// ceil(n / per_block) each, so block0 never decreases -- what find_job of repack.hip, the device half of the contract, relies on;
// upload() moves the table into an allocation of the gradient object and leaves dev / n / blocks, what the launch takes.  A
// load-params entry builds one locally and assigns it to its object once it is uploaded.
extern "C++" { // (a template, and functions that return C++ types, inside this file's extern "C")
template <class Job> struct JobTable {
    std::vector<Job> host;
    Job *dev = nullptr;
    int n = 0, blocks = 0;
    void add(Job job, int elems, int per_block) {
        job.block0 = blocks;
        blocks += (elems + per_block - 1) / per_block;
        host.push_back(job);
    }
    int upload(GradCore *g) {
        n = (int)host.size();
        if (n > 0) WSC_TRY(g->upload(host.data(), host.size() * sizeof(Job), (void **)&dev));
        host = std::vector<Job>();
        return WSC_OK;
    }
};
// `n` floats at `off` of the parameter buffer that a repack copies to `dst` as they are
void add_vec(JobTable<VecCopyJob> &vecs, long long off, int n, float *dst) { vecs.add({off, n, 0, dst}, n, VEC_COPY_PER_BLOCK); }
// the ops of a net's trunk that are convs, in op order: the layers the *_grad_create functions list first and the load-params
// entries rewrite
std::vector<size_t> trunk_conv_ops(const wsc_net *net) {
    std::vector<size_t> ops;
    for (size_t i = 0; i < net->ops.size(); ++i)
        if (net->ops[i].type == OP_CONV) ops.push_back(i);
    return ops;
}
// whether the net's conv `c` is the layer [k][k][Cin][Cout] of a layout (the first layer's 3 channels lie in the small form's 4)
bool conv_is_layer(const ConvW &c, int k, int Cin, int Cout) {
    return c.kh == k && c.kw == k && c.Cout == Cout && (c.form == CONV_FORM_GENERIC ? c.Cin == Cin : (c.Cin == 4 && Cin <= 4));
}
// the RepackJob of the net's conv `c`: its tensor [k][k][Cin][Cout] at w_off of the parameter buffer, its bias at b_off (-1: none),
// the data-gradient kernel it also rewrites (or null), cin_pad: the channels of its input where wider than the tensor
RepackJob conv_repack_job(const ConvW &c, int k, int Cin, int Cout, long long w_off, long long b_off, float *w_rot, int cin_pad = 0) {
    RepackJob J = RepackJob();
    J.w_off = w_off; J.b_off = b_off;
    J.k = k; J.Cin = Cin; J.Cout = Cout; J.Cin_pad = cin_pad;
    J.small = c.form != CONV_FORM_GENERIC;
    J.wp = c.w; J.s1 = c.s1; J.b1 = c.b1;
    J.w_rot = w_rot;
    return J;
}
} // extern "C++"
// the arguments every entry that takes a gradient object shares, checked before anything is launched (the workspace and the
// optimiser's scratch are the object's: one stream uses them, the one release() drains)
// (layout_elems: the size of the layout the entry's buffers are in where that is not the gradient layout -- wsc_cls_param_layout)
int grad_check(const char *fn, const wsc_ctx *ctx, const GradCore *g, long long elems, bool pointers_ok, long long layout_elems = -1) {
    WSC_CHECK(ctx && g && pointers_ok, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_CHECK(ctx == g->ctx, WSC_ERR_INVALID, "%s: the context is not the one the %s was created on", fn, g->kind);
    const long long want = layout_elems >= 0 ? layout_elems : g->grad_elems;
    WSC_CHECK(elems == want, WSC_ERR_INVALID, "%s: buffers of %lld floats, the layout has %lld", fn, elems, want);
    return WSC_OK;
}
// the workspace of GradCore::workspace in 256-byte lines
struct LineCarver {
    char *p;
    static size_t lines(long long elems) { return align_up((size_t)elems * sizeof(float), 256); }
    float *bytes(size_t n) { float *q = (float *)p; p += n; return q; }
    float *floats(long long elems) { return bytes(lines(elems)); }
};

struct GradLayer {
    std::string name;
    int k = 1, Cin = 0, Cout = 0, dil = 1;
    float *w_rot = nullptr; // the data-gradient kernel (dgrad_pack); null for the first layer: no gradient goes to the input
    long long w_off = 0, b_off = 0;
};
} // namespace
struct wsc_seg_grad : GradCore {
    using GradCore::GradCore;
    std::vector<GradLayer> layers; // the trunk's convs in op order, then fc6, fc7, fc8 of every branch
    std::vector<int> op_layer;     // layer of op i, -1 for a pool
    // the optimiser's view of the layout (sgd.hip): a segment per w and per b in offset order, built once; the partials and
    // the arrival counter of loss["l2"]
    SgdSegment *segs = nullptr;
    int n_segs = 0;
    double *l2_partials = nullptr;
    unsigned *l2_counter = nullptr;
};

void wsc_seg_grad_destroy(wsc_seg_grad *g) {
    if (!g) return;
    g->release();
    delete g;
}

int wsc_seg_grad_create(wsc_ctx *ctx, const wsc_net *net, const wsc_tensor_desc *weights, int n_weights, wsc_seg_grad **out) {
    WSC_CHECK(ctx && net && weights && out && n_weights > 0, WSC_ERR_INVALID, "wsc_seg_grad_create: null argument");
    WSC_TRY(need_seg("wsc_seg_grad_create", net));
    WSC_HIP(hipSetDevice(ctx->device));
    Dict d;
    WSC_TRY(descs_to_dict(weights, n_weights, &d));
    wsc_seg_grad *g = new wsc_seg_grad("wsc_seg_grad", ctx, net);
    auto fail = [&](int st) {
        wsc_seg_grad_destroy(g);
        return st;
    };
    int widest = 64;
    auto add = [&](const std::string &name, const ConvW &c, bool first) -> int {
        GradLayer L;
        L.name = name;
        L.k = c.kh; L.Cin = first ? 3 : c.Cin; L.Cout = c.Cout; L.dil = c.dil;
        auto wi = d.find(name + ".w");
        WSC_CHECK(wi != d.end() && wi->second.data != nullptr, WSC_ERR_SHAPE, "layer '%s': '%s.w' missing", name.c_str(), name.c_str());
        const HostTensor &w = wi->second;
        WSC_CHECK(w.ndim == 4 && w.shape[0] == L.k && w.shape[1] == L.k && w.shape[2] == L.Cin && w.shape[3] == L.Cout, WSC_ERR_SHAPE,
                  "layer '%s': '.w' must be HWIO [%d][%d][%d][%d] as the net has it, got ndim %d [%lld][%lld][%lld][%lld]", name.c_str(), L.k, L.k,
                  L.Cin, L.Cout, w.ndim, (long long)w.shape[0], (long long)w.shape[1], (long long)w.shape[2], (long long)w.shape[3]);
        WSC_CHECK(c.kh == c.kw && c.stride == 1 && c.pad == c.dil * (c.kh - 1) / 2 && (c.kh == 1 || c.kh == 3), WSC_ERR_INVALID,
                  "internal: layer '%s' is no stride-1 SAME convolution", name.c_str());
        if (!first) {
            std::vector<float> packed;
            dgrad_pack(w.data, L.k, L.Cin, L.Cout, &packed);
            WSC_TRY(g->upload(packed, &L.w_rot));
            widest = std::max(widest, conv_cout_pad(L.Cin));
        }
        L.w_off = g->grad_elems;
        g->grad_elems += (long long)L.k * L.k * L.Cin * L.Cout; // (no gaps: every float of the buffer is some layer's)
        L.b_off = g->grad_elems;
        g->grad_elems += L.Cout;
        g->layers.push_back(L);
        return WSC_OK;
    };
    g->op_layer.assign(net->ops.size(), -1);
    for (size_t i : trunk_conv_ops(net)) {
        g->op_layer[i] = (int)g->layers.size();
        const int st = add(net->ops[i].label, net->convs[net->ops[i].conv], i == 0);
        if (st != WSC_OK) return fail(st);
    }
    for (size_t k = 0; k < net->seg.size(); ++k) {
        const std::string sfx = net->seg.size() > 1 ? "_" + std::to_string(k + 1) : "";
        const ConvW *cs[3] = {&net->seg[k].fc6, &net->seg[k].fc7, &net->seg[k].fc8};
        for (int j = 0; j < 3; ++j) {
            const int st = add("fc" + std::to_string(6 + j) + sfx, *cs[j], false);
            if (st != WSC_OK) return fail(st);
        }
    }
    int st = g->ones_zeros(widest);
    if (st != WSC_OK) return fail(st);
    // the segment table of the optimiser: lr multipliers 1 (w) / 2 (b), 10 / 20 on fc8 (model.py:393-398, DSRG.py:434-439)
    std::vector<SgdSegment> segs;
    for (const GradLayer &L : g->layers) {
        const bool fc8 = L.name.compare(0, 3, "fc8") == 0;
        segs.push_back({L.w_off, fc8 ? 10.f : 1.f, 1});
        segs.push_back({L.b_off, fc8 ? 20.f : 2.f, 0});
    }
    if ((int)segs.size() > SGD_MAX_SEGMENTS || g->grad_elems >= (1ll << 31)) {
        wsc_set_error("wsc_seg_grad_create: %d layers, %lld parameters", (int)g->layers.size(), g->grad_elems);
        return fail(WSC_ERR_INVALID);
    }
    g->n_segs = (int)segs.size();
    st = g->upload(segs.data(), segs.size() * sizeof(SgdSegment), (void **)&g->segs);
    if (st == WSC_OK) st = g->zeroed(SGD_L2_MAX_BLOCKS * sizeof(double), (void **)&g->l2_partials);
    if (st == WSC_OK) st = g->zeroed(256, (void **)&g->l2_counter);
    if (st != WSC_OK) return fail(st);
    *out = g;
    return WSC_OK;
}

int wsc_seg_grad_layout(const wsc_seg_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *grad_elems_out) {
    WSC_CHECK(g && n_out && grad_elems_out && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_seg_grad_layout: null argument");
    *n_out = (int)g->layers.size();
    *grad_elems_out = g->grad_elems;
    for (int i = 0; i < max_entries && i < (int)g->layers.size(); ++i) {
        const GradLayer &L = g->layers[i];
        wsc_grad_entry e = {};
        std::strncpy(e.name, L.name.c_str(), sizeof(e.name) - 1);
        e.kh = e.kw = L.k; e.Cin = L.Cin; e.Cout = L.Cout;
        e.w_off = L.w_off; e.b_off = L.b_off;
        entries_out[i] = e;
    }
    return WSC_OK;
}

// wsc_net_backward_seg (fc_scale 1.0f) and wsc_net_backward_seg_drop (1 / (1 - drop_prob)): the same launches
static int backward_seg(const char *fn, wsc_ctx *ctx, wsc_seg_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                        const float *dfc8_dev, float *grad_dev, long long grad_elems, float fc_scale) {
    WSC_TRY(grad_check(fn, ctx, g, grad_elems, tape_dev && dfc8_dev && grad_dev));
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1, WSC_ERR_INVALID, "%s: B=%d input %d x %d", fn, B, H, W);
    const wsc_net *net = g->net;
    TapePlan tp;
    WSC_TRY(seg_tape_plan(net, B, H, W, &tp));
    WSC_TRY(tape_check(fn, "wsc_net_seg_tape_plan", tape_elems, tp.t));
    // every layer's plan and the workspace they need, before anything is launched
    const int hf = tp.pl.hf, wf = tp.pl.wf;
    const long long M8 = (long long)B * hf * wf;
    const size_t n_trunk = g->layers.size() - 3 * net->seg.size();
    std::vector<WgradPlan> plans(g->layers.size());
    long long g_max = 0, dz_max = M8 * dgrad_cz(net->C), slab_max = 0, part_max = 0;
    auto plan_layer = [&](size_t li, int h, int w) -> int {
        const GradLayer &L = g->layers[li];
        WSC_TRY(wgrad_plan(ctx, B, h, w, L.Cin, L.Cout, L.k, L.dil, 0, &plans[li]));
        const long long M = (long long)B * h * w;
        g_max = std::max(g_max, M * std::max(L.Cout, L.Cin));
        dz_max = std::max(dz_max, M * L.Cout);
        slab_max = std::max(slab_max, plans[li].slab_elems);
        part_max = std::max(part_max, (long long)relu_bias_grad_blocks(M) * L.Cout);
        return WSC_OK;
    };
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const OpDims &d = tp.pl.ops[i];
        g_max = std::max(g_max, (long long)B * d.H * d.W * d.C);
        if (g->op_layer[i] >= 0) WSC_TRY(plan_layer((size_t)g->op_layer[i], d.Ho, d.Wo));
    }
    for (size_t li = n_trunk; li < g->layers.size(); ++li) WSC_TRY(plan_layer(li, hf, wf));
    auto lines = LineCarver::lines;
    const long long sum_elems = M8 * net->F;
    WSC_TRY(g->workspace(2 * lines(g_max) + 2 * lines(sum_elems) + lines(dz_max) + lines(slab_max) + lines(part_max)));
    LineCarver ws = {(char *)g->ws};
    float *ga = ws.floats(g_max), *gb = ws.floats(g_max);
    float *gs[2] = {ws.floats(sum_elems), ws.floats(sum_elems)};
    float *dz = ws.floats(dz_max), *slab = ws.floats(slab_max), *partial = ws.floats(part_max);

    // one layer at gradient dy of its output [B][h][w][Cout]: db, dW, and (dx non-null) the gradient of its input; scale: 1.0f,
    // or the factor of the dropout site behind the layer (fc6 / fc7: y is then the dropped, scaled tape entry)
    auto layer_back = [&](size_t li, int h, int w, const float *x, const float *y /* null: no ReLU */, const float *dy, const float *sum_with,
                          float *dx, float scale = 1.0f) -> int {
        const GradLayer &L = g->layers[li];
        const long long M = (long long)B * h * w;
        const float *dzp = dy;
        if (y) {
            WSC_TRY(launch_relu_bias_grad(ctx, y, dy, M, L.Cout, scale, dz, partial, grad_dev + L.b_off));
            dzp = dz;
        } else {
            WSC_TRY(launch_relu_bias_grad(ctx, nullptr, dy, M, L.Cout, 1.0f, nullptr, partial, grad_dev + L.b_off));
        }
        WSC_TRY(wgrad_launch(ctx, plans[li], x, dzp, h, w, L.Cin, L.Cout, L.k, L.dil, slab, grad_dev + L.w_off));
        if (!dx) return WSC_OK;
        if (dgrad_cz(L.Cout) != L.Cout) { // (fc8: the class count padded to 32 input channels)
            WSC_TRY(launch_copy_channels(ctx, dzp, M, L.Cout, dgrad_cz(L.Cout), dz));
            dzp = dz;
        }
        return dgrad_launch(ctx, dzp, L.w_rot, g->ones, g->zeros, B, h, w, L.Cin, L.Cout, L.k, L.dil, sum_with, dx);
    };
    auto at = [&](int entry) { return tape_dev + tp.t.off(entry); };

    // the branches, _1 ... _4: each receives dfc8; their gradients into pool5a's output are summed in that order
    const int e_pool5a = tp.op_entry.back();
    for (size_t k = 0; k < net->seg.size(); ++k) {
        const size_t l6 = n_trunk + 3 * k;
        WSC_TRY(layer_back(l6 + 2, hf, wf, at(tp.fc7[k]), nullptr, dfc8_dev, nullptr, ga));
        WSC_TRY(layer_back(l6 + 1, hf, wf, at(tp.fc6[k]), at(tp.fc7[k]), ga, nullptr, gb, fc_scale));
        WSC_TRY(layer_back(l6, hf, wf, at(e_pool5a), at(tp.fc6[k]), gb, k > 0 ? gs[(k + 1) & 1] : nullptr, gs[k & 1], fc_scale));
    }
    // the trunk, last op first
    const float *gcur = gs[(net->seg.size() - 1) & 1];
    float *gfree[2] = {ga, gb};
    int nf = 0;
    for (int i = (int)net->ops.size() - 1; i >= 0; --i) {
        const Op &op = net->ops[i];
        const OpDims &d = tp.pl.ops[i];
        const float *x = at(i == 0 ? 0 : tp.op_entry[i - 1]);
        float *gout = gfree[nf];
        if (op.type == OP_POOL) {
            PoolGeom pg;
            WSC_CHECK(pool_geom(op.rule, op.pk, op.ps, op.pp, op.avg, d.H, d.W, &pg), WSC_ERR_INVALID, "internal: a pool plan_dims let through");
            WSC_TRY(launch_pool_grad(ctx, x, gcur, B, d.H, d.W, d.C, pg, gout));
        } else {
            WSC_TRY(layer_back((size_t)g->op_layer[i], d.Ho, d.Wo, x, at(tp.op_entry[i]), gcur, nullptr, i == 0 ? nullptr : gout));
        }
        gcur = gout;
        nf ^= 1;
    }
    return WSC_OK;
}

int wsc_net_backward_seg(wsc_ctx *ctx, wsc_seg_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                         const float *dfc8_dev, float *grad_dev, long long grad_elems) {
    return backward_seg("wsc_net_backward_seg", ctx, g, B, H, W, tape_dev, tape_elems, dfc8_dev, grad_dev, grad_elems, 1.0f);
}

int wsc_net_backward_seg_drop(wsc_ctx *ctx, wsc_seg_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                              const float *dfc8_dev, float *grad_dev, long long grad_elems, float drop_prob) {
    WSC_TRY(seg_dropout_check("wsc_net_backward_seg_drop", drop_prob, 0));
    return backward_seg("wsc_net_backward_seg_drop", ctx, g, B, H, W, tape_dev, tape_elems, dfc8_dev, grad_dev, grad_elems,
                        seg_dropout_scale(drop_prob));
}

// ---- the backward pass of the IRNet heads: d total / d edge_out, d total / d dp_out -> the gradient of every head parameter --------
// Every backbone stage is detached in Net.forward (resnet50_irn.py:111-115), so this is the whole gradient of a step.  The pass walks
// net->heads in reverse; the kernels are irn_grad.hip's, the GEMMs seg_grad.hip's.
namespace {
struct IrnGradHead {
    long long w_off = 0, g_off = 0, b_off = 0; // conv weight [Cin][Cout], GroupNorm weight, GroupNorm bias
    float *w_rot = nullptr;                    // the data-gradient kernel (dgrad_pack) of a head that reads a concat buffer
};
} // namespace
struct wsc_irn_grad : GradCore {
    using GradCore::GradCore;
    std::vector<IrnGradHead> heads; // one per net->heads
    long long edge_w_off = 0, edge_b_off = 0, dp_w_off = 0;
    long long dp_start = 0; // the first float of the dp group (train_irn.py:86-90: 10 lr); the edge group lies before it
    float *edge_rot = nullptr, *dp_rot = nullptr;
    JobTable<VecCopyJob> vecs; // the GroupNorm vectors of wsc_net_irn_load_params, built with its repack jobs
    std::vector<wsc_grad_entry> layout; // one entry per parameter, in the order of trainable_parameters()
};

void wsc_irn_grad_destroy(wsc_irn_grad *g) {
    if (!g) return;
    g->release();
    delete g;
}

int wsc_irn_grad_create(wsc_ctx *ctx, const wsc_net *net, const wsc_tensor_desc *weights, int n_weights, wsc_irn_grad **out) {
    WSC_CHECK(ctx && net && weights && out && n_weights > 0, WSC_ERR_INVALID, "wsc_irn_grad_create: null argument");
    WSC_TRY(need_irn("wsc_irn_grad_create", net));
    WSC_HIP(hipSetDevice(ctx->device));
    Dict d;
    WSC_TRY(descs_to_dict(weights, n_weights, &d));
    wsc_irn_grad *g = new wsc_irn_grad("wsc_irn_grad", ctx, net);
    g->heads.resize(net->heads.size());
    // `<name>` as torch has it, [Cout][Cin][1][1] (vec: [Cout]); the net's own tensor has that shape
    auto tensor = [&](const std::string &name, int Cout, int Cin, const HostTensor **t) -> int {
        auto it = d.find(name);
        WSC_CHECK(it != d.end() && it->second.data != nullptr, WSC_ERR_SHAPE, "layer '%s': missing", name.c_str());
        const HostTensor &w = it->second;
        const bool ok = Cin > 0 ? (w.ndim == 4 && w.shape[0] == Cout && w.shape[1] == Cin && w.shape[2] == 1 && w.shape[3] == 1)
                                : (w.ndim == 1 && w.shape[0] == Cout);
        WSC_CHECK(ok, WSC_ERR_SHAPE, "layer '%s': the net has it as [%d]%s, got ndim %d [%lld][%lld][%lld][%lld]", name.c_str(), Cout,
                  Cin > 0 ? ("[" + std::to_string(Cin) + "][1][1]").c_str() : "", w.ndim, (long long)w.shape[0], (long long)w.shape[1],
                  (long long)w.shape[2], (long long)w.shape[3]);
        *t = &w;
        return WSC_OK;
    };
    auto entry = [&](const std::string &name, int Cin, int Cout) {
        wsc_grad_entry e = {};
        std::strncpy(e.name, name.c_str(), sizeof(e.name) - 1);
        e.kh = e.kw = Cin > 0 ? 1 : 0;
        e.Cin = Cin; e.Cout = Cout;
        e.w_off = Cin > 0 ? g->grad_elems : -1;
        e.b_off = Cin > 0 ? -1 : g->grad_elems;
        g->layout.push_back(e);
        const long long at = g->grad_elems;
        g->grad_elems += Cin > 0 ? (long long)Cin * Cout : Cout; // (no gaps: every float of the buffer is some parameter's)
        return at;
    };
    int widest = 64;
    // the rotated kernel of a 1 x 1 layer [Cout][Cin] whose input has cin_pad >= Cin channels (zero rows beyond)
    auto rot = [&](const HostTensor *w, int Cin, int cin_pad, int Cout, float **dst) -> int {
        std::vector<float> hwio((size_t)cin_pad * Cout, 0.f), packed;
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < Cin; ++ci) hwio[(size_t)ci * Cout + co] = w->data[(size_t)co * Cin + ci];
        dgrad_pack(hwio.data(), 1, cin_pad, Cout, &packed);
        widest = std::max(widest, conv_cout_pad(cin_pad));
        return g->upload(packed, dst);
    };
    auto add_head = [&](size_t j) -> int {
        const IrnHead &h = net->heads[j];
        const HostTensor *w, *ga, *be;
        WSC_CHECK(h.conv.Cin % 64 == 0 && (h.src > 0 || (h.conv.stride == 1 && h.conv.Cout % 32 == 0)), WSC_ERR_INVALID,
                  "internal: head '%s' (%d -> %d channels, stride %d) has no backward form", h.name.c_str(), h.conv.Cin, h.conv.Cout, h.conv.stride);
        WSC_TRY(tensor(h.name + ".0.weight", h.conv.Cout, h.conv.Cin, &w));
        WSC_TRY(tensor(h.name + ".1.weight", h.conv.Cout, 0, &ga));
        WSC_TRY(tensor(h.name + ".1.bias", h.conv.Cout, 0, &be));
        if (h.src < 0) WSC_TRY(rot(w, h.conv.Cin, h.conv.Cin, h.conv.Cout, &g->heads[j].w_rot));
        g->heads[j].w_off = entry(h.name + ".0.weight", h.conv.Cin, h.conv.Cout);
        g->heads[j].g_off = entry(h.name + ".1.weight", 0, h.conv.Cout);
        g->heads[j].b_off = entry(h.name + ".1.bias", 0, h.conv.Cout);
        return WSC_OK;
    };
    auto build = [&]() -> int {
        // edge_layers: the heads of the edge concat, then the final edge conv; dp_layers: the other heads, then the final dp conv
        for (size_t j = 0; j < net->heads.size(); ++j)
            if (net->heads[j].dst == 0) WSC_TRY(add_head(j));
        const HostTensor *w6, *b6, *w7;
        WSC_TRY(tensor(net->edge_final + ".weight", 1, net->edge_in, &w6));
        WSC_TRY(tensor(net->edge_final + ".bias", 1, 0, &b6));
        WSC_TRY(rot(w6, net->edge_in, net->cats[0].channels, 1, &g->edge_rot));
        g->edge_w_off = entry(net->edge_final + ".weight", net->edge_in, 1);
        g->edge_b_off = entry(net->edge_final + ".bias", 0, 1);
        g->dp_start = g->grad_elems;
        for (size_t j = 0; j < net->heads.size(); ++j)
            if (net->heads[j].dst != 0) WSC_TRY(add_head(j));
        const int cd = net->cats.back().channels;
        WSC_TRY(tensor(net->dp_final + ".weight", 2, cd, &w7));
        WSC_TRY(rot(w7, cd, cd, 2, &g->dp_rot));
        g->dp_w_off = entry(net->dp_final + ".weight", cd, 2);
        return g->ones_zeros(widest);
    };
    const int st = build();
    if (st != WSC_OK) {
        wsc_irn_grad_destroy(g);
        return st;
    }
    *out = g;
    return WSC_OK;
}

int wsc_irn_grad_layout(const wsc_irn_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *grad_elems_out) {
    WSC_CHECK(g && n_out && grad_elems_out && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_irn_grad_layout: null argument");
    *n_out = (int)g->layout.size();
    *grad_elems_out = g->grad_elems;
    for (int i = 0; i < max_entries && i < (int)g->layout.size(); ++i) entries_out[i] = g->layout[i];
    return WSC_OK;
}

int wsc_net_backward_edge(wsc_ctx *ctx, wsc_irn_grad *g, int N, int S, const float *tape_dev, long long tape_elems, const float *dedge_dev,
                          const float *ddp_dev, float *grad_dev, long long grad_elems) {
    WSC_TRY(grad_check("wsc_net_backward_edge", ctx, g, grad_elems, tape_dev && dedge_dev && ddp_dev && grad_dev));
    WSC_CHECK(N > 0 && S > 0, WSC_ERR_INVALID, "wsc_net_backward_edge: N=%d S=%d", N, S);
    WSC_CHECK(((uintptr_t)tape_dev & 255) == 0, WSC_ERR_INVALID, "wsc_net_backward_edge: the tape must start on a 256-byte line");
    const wsc_net *net = g->net;
    EdgeTapePlan tp;
    WSC_TRY(edge_tape_plan(net, N, S, &tp));
    WSC_TRY(tape_check("wsc_net_backward_edge", "wsc_net_edge_tape_plan", tape_elems, tp.t));
    const EdgeGeom &eg = tp.g;
    const int NC = (int)net->cats.size(), NH = (int)net->heads.size();
    const long long Me = (long long)N * eg.He * eg.We, Md = (long long)N * eg.Hd * eg.Wd;
    // every GEMM's plan and the workspace, before anything is launched
    std::vector<WgradPlan> plans(NH);
    WgradPlan plan_e, plan_d;
    WSC_TRY(wgrad_plan(ctx, N, eg.He, eg.We, eg.cat_c[0], 2, 1, 1, 0, &plan_e)); // (two columns: column 1 is zeros, see below)
    WSC_TRY(wgrad_plan(ctx, N, eg.Hd, eg.Wd, eg.cat_c[NC - 1], 2, 1, 1, 0, &plan_d));
    long long dy_max = 0, dz_max = 32 * std::max(Me, Md), xs_max = 0, slab_max = std::max(plan_e.slab_elems, plan_d.slab_elems);
    size_t gpart_max = 0;
    int max_groups = 1;
    for (int j = 0; j < NH; ++j) {
        const IrnHead &h = net->heads[j];
        const EdgeGeom::Head &hg = eg.heads[j];
        WSC_TRY(wgrad_plan(ctx, N, hg.ho, hg.wo, h.conv.Cin, h.conv.Cout, 1, 1, 0, &plans[j]));
        const long long M = (long long)N * hg.ho * hg.wo;
        dy_max = std::max(dy_max, M * h.conv.Cout);
        if (h.conv.stride > 1) xs_max = std::max(xs_max, M * h.conv.Cin);
        slab_max = std::max(slab_max, plans[j].slab_elems);
        gpart_max = std::max(gpart_max, group_norm_grad_partial_bytes(N, hg.ho, hg.wo, h.conv.Cout));
        max_groups = std::max(max_groups, h.groups);
    }
    dz_max = std::max(dz_max, dy_max);
    auto lines = LineCarver::lines;
    const size_t gpart_bytes = align_up(gpart_max, 256), ms_bytes = align_up(sizeof(double) * 2 * N * max_groups, 256);
    size_t need = 2 * lines(dz_max) + lines(xs_max) + lines(slab_max) + lines(2 * std::max(Me, Md)) + lines(2 * eg.cat_c[0]) +
                  lines(relu_bias_grad_blocks(Me)) + gpart_bytes + ms_bytes;
    for (int i = 0; i < NC; ++i) need += lines((long long)eg.cat_elems[i]);
    WSC_TRY(g->workspace(need));
    LineCarver ws = {(char *)g->ws};
    float *dy = ws.floats(dz_max), *dz = ws.floats(dz_max); // (dz_max >= dy_max)
    float *xs = ws.floats(xs_max), *slab = ws.floats(slab_max), *two = ws.floats(2 * std::max(Me, Md));
    float *wtmp = ws.floats(2 * eg.cat_c[0]), *partial = ws.floats(relu_bias_grad_blocks(Me));
    void *gpart = ws.bytes(gpart_bytes), *ms = ws.bytes(ms_bytes);
    std::vector<float *> dcat(NC);
    for (int i = 0; i < NC; ++i) dcat[i] = ws.floats((long long)eg.cat_elems[i]);
    auto at = [&](int entry) { return tape_dev + tp.t.off(entry); };

    // the final edge conv (Cout = 1, bias): the GEMM takes two columns, d_edge and zeros, and column 0 of its result is dW; the
    // padding channels of the edge concat have no entry in the layout
    WSC_TRY(launch_copy_channels(ctx, dedge_dev, Me, 1, 2, two));
    WSC_TRY(wgrad_launch(ctx, plan_e, at(tp.cat[0]), two, eg.He, eg.We, eg.cat_c[0], 2, 1, 1, slab, wtmp));
    WSC_TRY(launch_copy_channels(ctx, wtmp, net->edge_in, 2, 1, grad_dev + g->edge_w_off));
    WSC_TRY(launch_relu_bias_grad(ctx, nullptr, dedge_dev, Me, 1, 1.0f, nullptr, partial, grad_dev + g->edge_b_off));
    WSC_TRY(launch_copy_channels(ctx, dedge_dev, Me, 1, dgrad_cz(1), dz));
    WSC_TRY(dgrad_launch(ctx, dz, g->edge_rot, g->ones, g->zeros, N, eg.He, eg.We, eg.cat_c[0], 1, 1, 1, nullptr, dcat[0]));
    // the final displacement conv (Cout = 2): dp_out's gradient comes channel-major
    WSC_TRY(launch_dp_to_nhwc(ctx, ddp_dev, N, eg.Hd * eg.Wd, dgrad_cz(2), dz));
    WSC_TRY(launch_copy_channels(ctx, dz, Md, dgrad_cz(2), 2, two));
    WSC_TRY(wgrad_launch(ctx, plan_d, at(tp.cat[NC - 1]), two, eg.Hd, eg.Wd, eg.cat_c[NC - 1], 2, 1, 1, slab, grad_dev + g->dp_w_off));
    WSC_TRY(dgrad_launch(ctx, dz, g->dp_rot, g->ones, g->zeros, N, eg.Hd, eg.Wd, eg.cat_c[NC - 1], 2, 1, 1, nullptr, dcat[NC - 1]));
    // the heads, last first: a concat buffer's reader ran after all of its writers, so its gradient is whole when they get here
    for (int j = NH - 1; j >= 0; --j) {
        const IrnHead &h = net->heads[j];
        const EdgeGeom::Head &hg = eg.heads[j];
        const IrnGradHead &gh = g->heads[j];
        const int di = h.dst, C = h.conv.Cout, Cin = h.conv.Cin;
        WSC_TRY(launch_relu_upsample_grad(ctx, dcat[di], at(tp.cat[di]), N, hg.ho, hg.wo, C, h.up, eg.cat_h[di], eg.cat_w[di], eg.cat_c[di], h.coff,
                                          dy));
        WSC_TRY(launch_group_norm_grad(ctx, at(tp.z[j]), at(tp.stats[j]), h.gamma, dy, N, hg.ho, hg.wo, C, h.groups, gpart, ms, dz,
                                       grad_dev + gh.g_off, grad_dev + gh.b_off));
        const int k = h.src > 0 ? h.src - 1 : -h.src - 1;
        const float *x = at(h.src > 0 ? tp.tap[k] : tp.cat[k]);
        if (h.conv.stride > 1) { // the pixels the strided 1 x 1 conv read, as a dense operand
            WSC_TRY(launch_strided_rows_f32(ctx, x, N, hg.sh, hg.sw, Cin, h.conv.stride, hg.ho, hg.wo, xs));
            x = xs;
        }
        WSC_TRY(wgrad_launch(ctx, plans[j], x, dz, hg.ho, hg.wo, Cin, C, 1, 1, slab, grad_dev + gh.w_off));
        // (stage taps are detached in the reference: no data gradient)
        if (h.src < 0) WSC_TRY(dgrad_launch(ctx, dz, gh.w_rot, g->ones, g->zeros, N, hg.ho, hg.wo, Cin, C, 1, 1, nullptr, dcat[k]));
    }
    return WSC_OK;
}

// ---- the update half of an IRNet step (train_irn.py:86-90, 127-129) and the closing dp_mean pass (148-164); kernels: sgd.hip,
// repack.hip, irn_grad.hip (the channel mean) -------------------------------------------------------------------------------------
int wsc_irn_sgd_step(wsc_ctx *ctx, wsc_irn_grad *g, float *param_dev, const float *grad_dev, float *mom_dev, long long elems, float lr_edge,
                     float lr_dp, float weight_decay, float sgd_momentum) {
    WSC_TRY(grad_check("wsc_irn_sgd_step", ctx, g, elems, param_dev && grad_dev && mom_dev));
    WSC_CHECK(std::isfinite(lr_edge) && std::isfinite(lr_dp) && std::isfinite(weight_decay) && std::isfinite(sgd_momentum), WSC_ERR_INVALID,
              "wsc_irn_sgd_step: lr_edge %g, lr_dp %g, weight_decay %g, sgd_momentum %g must be finite", (double)lr_edge, (double)lr_dp,
              (double)weight_decay, (double)sgd_momentum);
    WSC_HIP(hipSetDevice(ctx->device));
    return irn_sgd_launch(ctx, param_dev, grad_dev, mom_dev, elems, g->dp_start, lr_edge, lr_dp, weight_decay, sgd_momentum);
}

int wsc_net_irn_load_params(wsc_ctx *ctx, wsc_net *net, wsc_irn_grad *g, const float *param_dev, long long elems) {
    WSC_CHECK(ctx && net && g && param_dev, WSC_ERR_INVALID, "wsc_net_irn_load_params: null argument");
    WSC_TRY(need_irn("wsc_net_irn_load_params", net));
    WSC_CHECK(g->net == net, WSC_ERR_INVALID, "wsc_net_irn_load_params: the wsc_irn_grad was created for another net");
    WSC_TRY(grad_check("wsc_net_irn_load_params", ctx, g, elems, true));
    WSC_CHECK(g->heads.size() == net->heads.size(), WSC_ERR_INVALID, "internal: %d heads of the net, %d of the layout", (int)net->heads.size(),
              (int)g->heads.size());
    WSC_HIP(hipSetDevice(ctx->device));
    if (!g->repack.jobs_dev) { // the job tables: once per wsc_irn_grad (the packed buffers of both objects never move)
        std::vector<RepackJob> jobs; // 1 x 1 layers [Cin][Cout]
        JobTable<VecCopyJob> vecs;
        for (size_t j = 0; j < net->heads.size(); ++j) {
            const IrnHead &h = net->heads[j];
            const IrnGradHead &gh = g->heads[j];
            WSC_CHECK(h.conv.kh == 1 && h.conv.kw == 1 && h.conv.form == CONV_FORM_GENERIC && !h.conv.s2, WSC_ERR_INVALID,
                      "internal: head '%s' is no 1 x 1 layer", h.name.c_str());
            jobs.push_back(conv_repack_job(h.conv, 1, h.conv.Cin, h.conv.Cout, gh.w_off, -1, gh.w_rot));
            add_vec(vecs, gh.g_off, h.conv.Cout, h.gamma);
            add_vec(vecs, gh.b_off, h.conv.Cout, h.beta);
        }
        WSC_CHECK(net->edge6.Cin == net->cats[0].channels && net->edge6.Cout == 1 && net->dp7b.Cin == net->cats.back().channels &&
                      net->dp7b.Cout == 2,
                  WSC_ERR_INVALID, "internal: the final convs are not the layout's");
        WSC_CHECK(net->edge6.form == CONV_FORM_GENERIC && net->dp7b.form == CONV_FORM_GENERIC, WSC_ERR_INVALID, "internal: a final conv in the small form");
        jobs.push_back(conv_repack_job(net->edge6, 1, net->edge_in, 1, g->edge_w_off, g->edge_b_off, g->edge_rot, net->edge6.Cin));
        jobs.push_back(conv_repack_job(net->dp7b, 1, net->dp7b.Cin, 2, g->dp_w_off, -1, g->dp_rot));
        // (the vec-copy table first: jobs_dev, what marks the tables as built, is set last)
        WSC_TRY(vecs.upload(g));
        g->vecs = vecs;
        WSC_TRY(g->plan_repack(jobs));
    }
    WSC_TRY(repack_launch(ctx, g->repack, param_dev));
    return vec_copy_launch(ctx, g->vecs.dev, g->vecs.n, g->vecs.blocks, param_dev);
}

int wsc_channel_mean_nchw(wsc_ctx *ctx, const float *x_dev, int N, int C, int H, int W, const float *sub_host, double *out_dev) {
    WSC_CHECK(ctx && x_dev && out_dev, WSC_ERR_INVALID, "wsc_channel_mean_nchw: null argument");
    WSC_CHECK(N > 0 && C > 0 && C <= CHANNEL_MEAN_MAX_C && H > 0 && W > 0, WSC_ERR_INVALID, "wsc_channel_mean_nchw: %d x %d x %d x %d (C <= %d)",
              N, C, H, W, CHANNEL_MEAN_MAX_C);
    WSC_CHECK(((uintptr_t)x_dev & 3) == 0 && ((uintptr_t)out_dev & 7) == 0, WSC_ERR_INVALID,
              "wsc_channel_mean_nchw: x_dev must be 4-byte and out_dev 8-byte aligned");
    WSC_HIP(hipSetDevice(ctx->device));
    return channel_mean_launch(ctx, x_dev, N, C, (long long)H * W, sub_host, out_dev);
}

int wsc_net_set_mean_shift(wsc_net *net, const float m[2]) {
    WSC_CHECK(net && m, WSC_ERR_INVALID, "wsc_net_set_mean_shift: null argument");
    WSC_CHECK(!net->heads.empty(), WSC_ERR_INVALID, "wsc_net_set_mean_shift: the network is not an IRNet EdgeDisplacement net");
    WSC_CHECK(std::isfinite(m[0]) && std::isfinite(m[1]), WSC_ERR_INVALID, "wsc_net_set_mean_shift: (%g, %g) is not finite", (double)m[0],
              (double)m[1]);
    net->mean_shift[0] = m[0];
    net->mean_shift[1] = m[1];
    return WSC_OK;
}

int wsc_net_get_mean_shift(const wsc_net *net, float m_out[2]) {
    WSC_CHECK(net && m_out, WSC_ERR_INVALID, "wsc_net_get_mean_shift: null argument");
    WSC_CHECK(!net->heads.empty(), WSC_ERR_INVALID, "wsc_net_get_mean_shift: the network is not an IRNet EdgeDisplacement net");
    m_out[0] = net->mean_shift[0];
    m_out[1] = net->mean_shift[1];
    return WSC_OK;
}

// ---- the update half of the training step: Model.optimize() (model.py:379-404) on the layout of wsc_seg_grad_layout ----------------
int wsc_seg_sgd_accumulate(wsc_ctx *ctx, wsc_seg_grad *g, const float *param_dev, const float *grad_dev, float *accum_dev, long long elems,
                           float weight_decay, int accum_num, float *l2_dev) {
    WSC_TRY(grad_check("wsc_seg_sgd_accumulate", ctx, g, elems, param_dev && grad_dev && accum_dev));
    WSC_CHECK(accum_num >= 1, WSC_ERR_INVALID, "wsc_seg_sgd_accumulate: accum_num=%d", accum_num);
    WSC_HIP(hipSetDevice(ctx->device));
    return sgd_accumulate_launch(ctx, g->segs, g->n_segs, param_dev, grad_dev, accum_dev, elems, weight_decay, accum_num, g->l2_partials,
                                 g->l2_counter, l2_dev);
}

int wsc_seg_sgd_apply(wsc_ctx *ctx, wsc_seg_grad *g, float *param_dev, float *accum_dev, float *mom_dev, long long elems, float lr,
                      float momentum, int clear_accum) {
    WSC_TRY(grad_check("wsc_seg_sgd_apply", ctx, g, elems, param_dev && accum_dev && mom_dev));
    WSC_HIP(hipSetDevice(ctx->device));
    return sgd_apply_launch(ctx, param_dev, accum_dev, mom_dev, elems, lr, momentum, clear_accum);
}

int wsc_net_seg_load_params(wsc_ctx *ctx, wsc_net *net, wsc_seg_grad *g, const float *param_dev, long long elems) {
    WSC_CHECK(ctx && net && g && param_dev, WSC_ERR_INVALID, "wsc_net_seg_load_params: null argument");
    WSC_TRY(need_seg("wsc_net_seg_load_params", net));
    WSC_CHECK(g->net == net, WSC_ERR_INVALID, "wsc_net_seg_load_params: the wsc_seg_grad was created for another net");
    WSC_TRY(grad_check("wsc_net_seg_load_params", ctx, g, elems, true));
    // the layers in the order wsc_seg_grad_create listed them: the trunk's convs in op order, then fc6, fc7, fc8 of every branch
    std::vector<ConvW *> convs;
    for (size_t i : trunk_conv_ops(net)) convs.push_back(&net->convs[net->ops[i].conv]);
    for (SegBranch &br : net->seg) {
        convs.push_back(&br.fc6);
        convs.push_back(&br.fc7);
        convs.push_back(&br.fc8);
    }
    WSC_CHECK(convs.size() == g->layers.size(), WSC_ERR_INVALID, "internal: %d layers of the net, %d of the layout", (int)convs.size(),
              (int)g->layers.size());
    for (size_t i = 0; i < convs.size(); ++i) {
        const ConvW &c = *convs[i];
        const GradLayer &L = g->layers[i];
        WSC_CHECK(conv_is_layer(c, L.k, L.Cin, L.Cout) && !c.s2 && !c.b2, WSC_ERR_INVALID, "internal: layer '%s' of the layout is not the net's",
                  L.name.c_str());
    }
    WSC_HIP(hipSetDevice(ctx->device));
    if (!g->repack.jobs_dev) { // the job table: once per wsc_seg_grad (the packed buffers of both objects never move)
        std::vector<RepackJob> jobs;
        for (size_t i = 0; i < convs.size(); ++i) {
            const GradLayer &L = g->layers[i];
            jobs.push_back(conv_repack_job(*convs[i], L.k, L.Cin, L.Cout, L.w_off, L.b_off, L.w_rot));
        }
        WSC_TRY(g->plan_repack(jobs));
    }
    return repack_launch(ctx, g->repack, param_dev);
}

// One convolution layer through the production kernel, NCHW fp32 in / out (layout changes and
// weight packing included): y = [relu]( conv(x, w) * scale + shift [+ residual] ).
int wsc_conv2d_nchw(wsc_ctx *ctx, const float *x_dev, int N, int Cin, int H, int W, const float *w_host, int Cout,
                    int kh, int kw, int stride, int pad, const float *scale_host, const float *shift_host,
                    const float *residual_dev, int relu, int precision, float *y_dev) {
    return wsc_conv2d_nchw_dil(ctx, x_dev, N, Cin, H, W, w_host, Cout, kh, kw, stride, pad, 1, scale_host, shift_host, residual_dev, relu,
                               precision, y_dev);
}

int wsc_conv2d_nchw_dil(wsc_ctx *ctx, const float *x_dev, int N, int Cin, int H, int W, const float *w_host, int Cout, int kh, int kw,
                        int stride, int pad, int dil, const float *scale_host, const float *shift_host, const float *residual_dev,
                        int relu, int precision, float *y_dev) {
    WSC_CHECK(ctx && x_dev && w_host && y_dev, WSC_ERR_INVALID, "wsc_conv2d_nchw: null argument");
    WSC_CHECK(dil >= 1 && (dil == 1 || (Cin > 4 && stride >= 1)), WSC_ERR_INVALID,
              "wsc_conv2d_nchw: dilation %d (>= 1; > 1 on the generic form only, Cin a multiple of 64)", dil);
    WSC_CHECK(Cout % 8 == 0, WSC_ERR_INVALID, "wsc_conv2d_nchw: Cout=%d must be a multiple of 8", Cout);
    WSC_HIP(hipSetDevice(ctx->device));
    wsc_net tmp;
    tmp.ctx = ctx;
    const int generic = (precision & WSC_CONV_GENERIC) ? 1 : 0;
    wsc_precision prec;
    WSC_TRY(decode_precision(precision & ~WSC_CONV_GENERIC, &prec));
    tmp.prec = prec;
    HostTensor wt;
    wt.data = w_host; wt.ndim = 4; wt.shape[0] = Cout; wt.shape[1] = Cin; wt.shape[2] = kh; wt.shape[3] = kw;
    std::vector<float> s1(Cout, 1.f), b1(Cout, 0.f);
    if (scale_host) s1.assign(scale_host, scale_host + Cout);
    if (shift_host) b1.assign(shift_host, shift_host + Cout);
    ConvForm form = CONV_FORM_GENERIC;
    if (Cin <= 4) form = kw <= 4 ? CONV_FORM_SMALL2 : CONV_FORM_SMALL4;
    if (form == CONV_FORM_SMALL4 && conv_split(prec) == 2 && (stride & 1) == 0 && kw <= 7) form = CONV_FORM_STEM_ROWS; // (padded input)
    ConvW c;
    int st = make_conv(&tmp, &wt, stride, pad, relu, form, s1, b1, nullptr, nullptr, &c);
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : tmp.allocs) (void)hipFree(p);
    };
    if (st != WSC_OK) { cleanup(); return st; }
    c.dil = dil;
    const int Ho = (H + 2 * pad - ((kh - 1) * dil + 1)) / stride + 1, Wo = (W + 2 * pad - ((kw - 1) * dil + 1)) / stride + 1;
    if (Ho < 1 || Wo < 1) {
        cleanup();
        wsc_set_error("wsc_conv2d_nchw: a %d x %d input is too small for this kernel, padding and dilation", H, W);
        return WSC_ERR_INVALID;
    }
    int in_h = H, in_w = W;
    if (form == CONV_FORM_STEM_ROWS) conv_stem_rows_input_dims(Ho, Wo, stride, kh, &in_h, &in_w);
    const size_t in_e = (size_t)N * in_h * in_w * c.Cin, out_e = (size_t)N * Ho * Wo * Cout;
    void *ws;
    st = wsc_ctx_workspace(ctx, act_bytes(in_e, prec) + 2 * act_bytes(out_e, prec), &ws);
    if (st != WSC_OK) { cleanup(); return st; }
    char *p = (char *)ws;
    const Act xi = act_carve(p, in_e, prec), yo = act_carve(p, out_e, prec);
    const Act ri = residual_dev ? act_carve(p, out_e, prec) : Act();
    // (the small-Cin forms multiply a zero-weighted extra pixel per kernel row: 0 * NaN would spread a non-finite input beyond the
    // cells that read it, so in the 16-bit modes their input is loud in bf16 / bf16x3 as well)
    unsigned *door = layer_door(ctx, prec);
    unsigned *door_x = (form != CONV_FORM_GENERIC && prec != WSC_PREC_F32) ? ctx->range_dev : door;
    if (form == CONV_FORM_STEM_ROWS) st = launch_nchw_to_nhwc4_pad(ctx, x_dev, N, H, W, in_h, in_w, pad, xi, door_x);
    else if (form != CONV_FORM_GENERIC) st = launch_nchw_to_nhwc4(ctx, x_dev, N, H, W, xi, door_x);
    else st = launch_nchw_to_nhwc(ctx, x_dev, N, Cin, H * W, xi, door);
    if (st == WSC_OK && residual_dev) st = launch_nchw_to_nhwc(ctx, residual_dev, N, Cout, Ho * Wo, ri, door);
    if (st == WSC_OK) {
        ConvLaunch L = conv_launch(c, prec);
        L.x = xi; L.res = ri; L.y = yo;
        L.N = N; L.H = H; L.W = W; L.Ho = Ho; L.Wo = Wo;
        if (form == CONV_FORM_STEM_ROWS) on_padded_input(L, in_h, in_w);
        L.generic = generic;
        st = conv_igemm_launch(ctx, L);
    }
    if (st == WSC_OK) st = launch_nhwc_to_nchw(ctx, yo, N, Cout, Ho * Wo, y_dev);
    cleanup();
    return st;
}

// ---- single layers of the nets for the per-layer tests (tests/test_gpu_layers.py): fp32 in and out, the values staged into an
// activation of `precision` with the layout change of the entries above (one "pixel" per row: the layout stays, the values take
// the planes), then the PRODUCTION launcher, unchanged.  Every argument is checked before anything is launched.
int wsc_group_norm_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, const float *gamma_host, const float *beta_host,
                        int G, float eps, int up, int relu, int Hd, int Wd, int Ctot, int coff, int precision, float *y_dev) {
    WSC_CHECK(ctx && x_dev && gamma_host && beta_host && y_dev, WSC_ERR_INVALID, "wsc_group_norm_nhwc: null argument");
    wsc_precision prec;
    WSC_TRY(decode_precision(precision, &prec));
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && G > 0 && C % G == 0, WSC_ERR_INVALID,
              "wsc_group_norm_nhwc: %d x %d x %d x %d in %d groups", N, H, W, C, G);
    WSC_CHECK(up == 1 || up == 2 || up == 4, WSC_ERR_INVALID, "wsc_group_norm_nhwc: upsample factor %d (1, 2 or 4)", up);
    WSC_CHECK(Hd >= 1 && Wd >= 1 && Hd <= H * up && Wd <= W * up, WSC_ERR_INVALID,
              "wsc_group_norm_nhwc: crop %d x %d of a %d x %d map", Hd, Wd, H * up, W * up);
    WSC_CHECK(coff >= 0 && Ctot >= 1 && coff <= Ctot - C, WSC_ERR_INVALID, "wsc_group_norm_nhwc: channels [%d, %d + %d) of %d", coff, coff, C,
              Ctot);
    WSC_CHECK(prec != WSC_PREC_F32 || (C % 4 == 0 && Ctot % 4 == 0 && coff % 4 == 0 && ((uintptr_t)x_dev & 15) == 0), WSC_ERR_INVALID,
              "wsc_group_norm_nhwc (fp32): %d of %d channels at %d are not 16-byte groups", C, Ctot, coff);
    WSC_HIP(hipSetDevice(ctx->device));
    const size_t out_e = (size_t)N * Hd * Wd * Ctot;
    const size_t part_b = align_up(group_norm_partial_bytes(N, H, W, G), 256), stats_b = align_up(sizeof(float) * 2 * N * G, 256),
                 vec_b = align_up(sizeof(float) * C, 256);
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, act_bytes(out_e, prec) + part_b + stats_b + 2 * vec_b, &ws));
    char *p = (char *)ws;
    const Act yo = act_carve(p, out_e, prec);
    void *part = p, *stats = p + part_b;
    float *gamma = (float *)(p + part_b + stats_b), *beta = (float *)(p + part_b + stats_b + vec_b);
    WSC_TRY(wsc_ctx_upload_small(ctx, gamma, gamma_host, sizeof(float) * C));
    WSC_TRY(wsc_ctx_upload_small(ctx, beta, beta_host, sizeof(float) * C));
    WSC_TRY(launch_nchw_to_nhwc(ctx, y_dev, N * Hd * Wd, Ctot, 1, yo, nullptr)); // (no door: it may be scratch -- what the other heads of the concat buffer wrote)
    WSC_TRY(launch_group_norm_stats(ctx, x_dev, N, H, W, C, G, eps, part, stats));
    WSC_TRY(launch_group_norm_apply(ctx, x_dev, stats, gamma, beta, N, H, W, C, G, up, relu, yo, Hd, Wd, Ctot, coff));
    return launch_act_to_f32(ctx, yo, out_e, y_dev);
}

int wsc_gap_linear_sigmoid(wsc_ctx *ctx, const float *feat_dev, int B, int hw, int F, const float *w_host, const float *bias_host, int C,
                           int sample_stride, int precision, float *score_dev) {
    WSC_CHECK(ctx && feat_dev && w_host && score_dev, WSC_ERR_INVALID, "wsc_gap_linear_sigmoid: null argument");
    wsc_precision prec;
    WSC_TRY(decode_precision(precision, &prec));
    WSC_CHECK(B > 0 && hw != 0 && hw > -(1 << 24) && hw < (1 << 24) && F > 0 && F <= 8192 && C > 0 && sample_stride >= 1 && sample_stride <= 2,
              WSC_ERR_INVALID, "wsc_gap_linear_sigmoid: B=%d, %d positions, F=%d, C=%d, sample stride %d", B, hw, F, C, sample_stride);
    WSC_HIP(hipSetDevice(ctx->device));
    const int npix = hw < 0 ? -hw : hw;
    const size_t in_e = (size_t)B * sample_stride * npix * F;
    const size_t w_b = align_up(sizeof(float) * (size_t)C * F, 256), b_b = align_up(sizeof(float) * C, 256);
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, act_bytes(in_e, prec) + w_b + b_b, &ws));
    char *p = (char *)ws;
    const Act feat = act_carve(p, in_e, prec);
    float *w = (float *)p, *bias = bias_host ? (float *)(p + w_b) : nullptr;
    WSC_TRY(wsc_ctx_upload_small(ctx, w, w_host, sizeof(float) * (size_t)C * F));
    if (bias) WSC_TRY(wsc_ctx_upload_small(ctx, bias, bias_host, sizeof(float) * C));
    WSC_TRY(launch_nchw_to_nhwc(ctx, feat_dev, B * sample_stride * npix, F, 1, feat, layer_door(ctx, prec)));
    return launch_gap_linear_sigmoid(ctx, feat, B, hw, F, w, bias, C, score_dev, sample_stride);
}

int wsc_cam_flip_add(wsc_ctx *ctx, const float *head_dev, int B, int h, int w, int C, int Cs, float *cam_dev) {
    WSC_CHECK(ctx && head_dev && cam_dev, WSC_ERR_INVALID, "wsc_cam_flip_add: null argument");
    WSC_CHECK(B > 0 && h > 0 && w > 0 && C > 0 && C <= Cs, WSC_ERR_INVALID, "wsc_cam_flip_add: B=%d, %d x %d, %d of %d channels", B, h, w, C, Cs);
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_flip_add(ctx, head_dev, B, h, w, C, Cs, cam_dev);
}

int wsc_irn_edge_finish(wsc_ctx *ctx, const float *e_dev, int He, int We, const float *d_dev, int Hd, int Wd, int B, int fh, int fw,
                        float ms0, float ms1, float *edge_dev, float *dp_dev) {
    WSC_CHECK(ctx && e_dev && d_dev && edge_dev && dp_dev, WSC_ERR_INVALID, "wsc_irn_edge_finish: null argument");
    WSC_CHECK(B > 0 && fh > 0 && fw > 0, WSC_ERR_INVALID, "wsc_irn_edge_finish: B=%d, feature size %d x %d", B, fh, fw);
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_edge_finish(ctx, e_dev, He, We, d_dev, Hd, Wd, B, fh, fw, ms0, ms1, edge_dev, dp_dev); // (checks fh, fw against the maps)
}

// ---- 01_train: the plain stacks (VGG16 / M7) in training mode, and their backward pass ------------------------------------------
// The graph is common_cnn.make_layers': conv(bias) -> ReLU -> BatchNorm(eps = 1e-3) per entry, the pools between, the `D` entries of
// VGG16's layer5 and of M7's classifier branch the identity in wsc_net_forward_cls_train / wsc_net_backward_cls and the sites of
// the *_drop entry points (Op::drop_site, M7_DROP_SITE; the contract: dropout_rng.h).  wsc_cls_loss hands out d loss / d feat on
// the last feature map; the pass below carries it to every conv and BatchNorm parameter.  Kernels: cls_grad.hip (BatchNorm),
// pool.hip, seg_grad.hip (the GEMMs).
namespace {
int need_cls(const char *fn, const wsc_net *net) {
    WSC_CHECK(net->arch == WSC_ARCH_VGG16_CAM || net->arch == WSC_ARCH_M7_CAM, WSC_ERR_INVALID,
              "%s: the network is not a WSC_ARCH_VGG16_CAM / WSC_ARCH_M7_CAM net", fn);
    return WSC_OK;
}
// "input"; per conv "<key>" (its post-ReLU output) and, with BatchNorm, "<key>.bn" (the normalised output) and "<key>.stats"
// ([1][1][1][2 C] {mean, rstd} pairs); "pool:<i>" -- each the value the next op read
struct ClsTapePlan {
    Plan pl;
    TapeLayout t;
    std::vector<int> a, stats, out; // per op: the conv's post-ReLU entry and its statistics (-1 without), the entry the next op read
};
int cls_tape_plan(const wsc_net *net, int B, int H, int W, ClsTapePlan *tp) {
    WSC_TRY(plan_dims(net, B, H, W, &tp->pl));
    tp->t.add("input", B, H, W, 3);
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const Op &op = net->ops[i];
        const OpDims &d = tp->pl.ops[i];
        WSC_CHECK(op.type != OP_GATHER && op.res < 0 && op.in2 < 0 && op.pitch == 0 && (i == 0 ? op.in < 0 : op.in == net->ops[i - 1].out) &&
                      !(op.type == OP_POOL && op.avg),
                  WSC_ERR_INVALID, "internal: op %d of a plain stack is no link of a chain", (int)i);
        const int first = tp->t.add(op.label, B, d.Ho, d.Wo, d.Co);
        const bool bn = op.type == OP_CONV && net->convs[op.conv].bn >= 0;
        tp->a.push_back(op.type == OP_CONV ? first : -1);
        tp->out.push_back(bn ? tp->t.add(op.label + ".bn", B, d.Ho, d.Wo, d.Co) : first);
        tp->stats.push_back(bn ? tp->t.add(op.label + ".stats", 1, 1, 1, 2 * d.Co) : -1);
    }
    return WSC_OK;
}
int cls_shape_check(const char *fn, int B, int H, int W, const float *tape_dev) {
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1, WSC_ERR_INVALID, "%s: B=%d input %d x %d", fn, B, H, W);
    WSC_CHECK(((uintptr_t)tape_dev & 255) == 0, WSC_ERR_INVALID, "%s: the tape must start on a 256-byte line", fn);
    return WSC_OK;
}
// M7's classifier branch (layer3_p2: MaxPool2d(2, 2), or the third row of `pool_spec`) on the hf x wf feature map
int cls_branch_pool(const char *fn, const wsc_net *net, int hf, int wf, PoolGeom *g) {
    const bool ok = net->cls_pool_set ? pool_geom(net->cls_pool.rule(), net->cls_pool.k, net->cls_pool.stride, 0, false, hf, wf, g)
                                      : pool_geom(POOL_TORCH, 2, 2, 0, false, hf, wf, g);
    WSC_CHECK(ok, WSC_ERR_INVALID, "%s: the %d x %d feature map is smaller than the classifier branch's pool", fn, hf, wf);
    return WSC_OK;
}
// the map wsc_cls_loss reduces: the last feature map -- or, with M7's dropout site active, the pooled map the site drops
int cls_feat_dims(const char *fn, const wsc_net *net, const Plan &pl, bool dropping, int *h, int *w) {
    *h = pl.hf;
    *w = pl.wf;
    if (!dropping || !net->cls_max) return WSC_OK;
    PoolGeom g;
    WSC_TRY(cls_branch_pool(fn, net, pl.hf, pl.wf, &g));
    *h = g.Ho;
    *w = g.Wo;
    return WSC_OK;
}
constexpr unsigned M7_DROP_SITE = 0; // the one 'D' entry of m7.py:41, behind layer3_p2
} // namespace

int wsc_net_cls_feat_dims(const wsc_net *net, int H, int W, int dropping, int *h, int *w) {
    const char *fn = "wsc_net_cls_feat_dims";
    WSC_CHECK(net && h && w, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_TRY(need_cls(fn, net));
    WSC_CHECK(H >= 1 && W >= 1, WSC_ERR_INVALID, "%s: input %d x %d", fn, H, W);
    Plan pl;
    WSC_TRY(plan_dims(net, 1, H, W, &pl));
    return cls_feat_dims(fn, net, pl, dropping != 0, h, w);
}

int wsc_net_cls_tape_plan(wsc_ctx *ctx, const wsc_net *net, int B, int H, int W, wsc_tape_entry *entries_out, int max_entries, int *n_out,
                          long long *tape_elems_out) {
    WSC_CHECK(ctx && net && n_out && tape_elems_out, WSC_ERR_INVALID, "wsc_net_cls_tape_plan: null argument");
    WSC_TRY(need_cls("wsc_net_cls_tape_plan", net));
    WSC_CHECK(B >= 1 && H >= 1 && W >= 1 && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_net_cls_tape_plan: B=%d input %d x %d, room for %d entries", B, H, W, max_entries);
    ClsTapePlan tp;
    WSC_TRY(cls_tape_plan(net, B, H, W, &tp));
    return tape_export(tp.t, entries_out, max_entries, n_out, tape_elems_out);
}

namespace {
// wsc_net_forward_cls_train (drop null) and wsc_net_forward_cls_train_drop (drop null at drop_prob = 0: the same launches)
int cls_forward(const char *fn, wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float keep, int unbiased,
                float *run_dev, float *tape_dev, long long tape_elems, float *feat_dev, const long long *feat_elems, const ClsDrop *drop) {
    WSC_CHECK(ctx && net && x_dev && tape_dev && feat_dev, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_TRY(need_cls(fn, net));
    WSC_TRY(cls_shape_check(fn, B, H, W, tape_dev));
    WSC_CHECK(keep >= 0.f && keep <= 1.f && (unbiased == 0 || unbiased == 1), WSC_ERR_INVALID,
              "%s: keep = %g (the weight of the old running value, 0 .. 1), unbiased = %d (0 / 1)", fn, (double)keep, unbiased);
    ClsTapePlan tp;
    WSC_TRY(cls_tape_plan(net, B, H, W, &tp));
    WSC_TRY(tape_check(fn, "wsc_net_cls_tape_plan", tape_elems, tp.t));
    int h_out, w_out;
    WSC_TRY(cls_feat_dims(fn, net, tp.pl, drop != nullptr, &h_out, &w_out));
    WSC_CHECK(!feat_elems || *feat_elems == (long long)B * h_out * w_out * net->F, WSC_ERR_INVALID,
              "%s: feat_elems = %lld, the map is [%d][%d][%d][%d] (wsc_net_cls_feat_dims)", fn, feat_elems ? *feat_elems : 0ll, B, h_out, w_out, net->F);
    std::vector<long long> a_off, stats_off, y_off;
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const OpDims &d = tp.pl.ops[i];
        WSC_CHECK(!(unbiased && tp.stats[i] >= 0 && (long long)B * d.Ho * d.Wo == 1), WSC_ERR_INVALID,
                  "%s: BatchNorm '%s' sees one value per channel: the unbiased running variance needs more", fn, net->ops[i].label.c_str());
        a_off.push_back(tp.t.off(tp.a[i] >= 0 ? tp.a[i] : tp.out[i])); // (what the op itself wrote)
        stats_off.push_back(tp.stats[i] >= 0 ? tp.t.off(tp.stats[i]) : -1);
        y_off.push_back(tp.t.off(tp.out[i]));
    }
    WSC_HIP(hipSetDevice(ctx->device));
    const TraceSink sink = {a_off.data(), tape_dev};
    const BnTrainSink bn = {a_off.data(), stats_off.data(), y_off.data(), tape_dev, keep, unbiased, run_dev, drop};
    // (behind the stack's buffers: the NHWC4 input as fp32 on its way to the tape's 3-channel entry)
    const size_t in4_elems = (size_t)B * H * W * 4;
    Act feat, xin, spare;
    int hf, wf;
    void *extra;
    WSC_TRY(run_backbone(ctx, net, x_dev, B, H, in4_elems * sizeof(float), &feat, &hf, &wf, &extra, nullptr, W, false, &spare, &sink, &xin, &bn));
    WSC_TRY(launch_act_to_f32(ctx, xin, in4_elems, (float *)extra));
    WSC_TRY(launch_copy_channels(ctx, (const float *)extra, (long long)B * H * W, 4, 3, tape_dev + tp.t.off(0)));
    if (drop && net->cls_max) { // M7: layer3_p2 -> the site -> (wsc_cls_loss's) global max; the pooled map is dropped as fp32
        PoolGeom g;
        WSC_TRY(cls_branch_pool(fn, net, hf, wf, &g));
        const long long n = (long long)B * g.Ho * g.Wo * net->F;
        WSC_TRY(launch_pool(ctx, feat, B, hf, wf, net->F, g, spare));
        WSC_TRY(launch_act_to_f32(ctx, spare, (size_t)n, feat_dev));
        return launch_seg_dropout_f32(ctx, feat_dev, feat_dev, nullptr, nullptr, n, 0ull, drop->drop_prob, drop->seed, drop->step, M7_DROP_SITE);
    }
    return launch_act_to_f32(ctx, feat, (size_t)B * hf * wf * net->F, feat_dev);
}
} // namespace

int wsc_net_forward_cls_train(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float keep, int unbiased,
                              float *run_dev, float *tape_dev, long long tape_elems, float *feat_dev) {
    return cls_forward("wsc_net_forward_cls_train", ctx, net, x_dev, B, H, W, keep, unbiased, run_dev, tape_dev, tape_elems, feat_dev, nullptr,
                       nullptr);
}

int wsc_net_forward_cls_train_drop(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float keep, int unbiased,
                                   float *run_dev, float *tape_dev, long long tape_elems, float *feat_dev, long long feat_elems, float drop_prob,
                                   unsigned long long seed, long long step) {
    const char *fn = "wsc_net_forward_cls_train_drop";
    WSC_TRY(seg_dropout_check(fn, drop_prob, step));
    const ClsDrop drop = {drop_prob, seed, (unsigned)step};
    return cls_forward(fn, ctx, net, x_dev, B, H, W, keep, unbiased, run_dev, tape_dev, tape_elems, feat_dev, &feat_elems,
                       drop_prob > 0.f ? &drop : nullptr);
}

namespace {
struct ClsGradLayer {
    int Cin = 0, Cout = 0, bn = -1;
    float *w_rot = nullptr; // the data-gradient kernel (dgrad_pack); null for the first layer: no gradient goes to the input
    long long w_off = 0, b_off = 0, g_off = -1, be_off = -1; // conv weight [3][3][Cin][Cout], conv bias, BatchNorm weight, BatchNorm bias
};
} // namespace
struct wsc_cls_grad : GradCore {
    using GradCore::GradCore;
    std::vector<ClsGradLayer> layers;   // the convs in op order
    std::vector<int> op_layer;          // layer of op i, -1 for a pool
    std::vector<wsc_grad_entry> layout; // one entry per parameter, in plain_module_order
    // the training layout (wsc_cls_param_layout): the gradient layout, then the classifier's Linear [C][F] and its bias
    long long param_elems = 0, cls_w_off = 0, cls_b_off = -1;
    // wsc_net_cls_load_params, built by its first call with the repack jobs: BatchNorm's gamma / beta and the classifier's fp32
    // copies (a vec-copy table), the inference folds, the CAM head (the transposed Linear in `head_t`, a repack plan of its own)
    JobTable<VecCopyJob> vecs;
    JobTable<BnFoldJob> folds;
    float *head_t = nullptr; // [F][C]
    RepackPlan head_repack;
};

void wsc_cls_grad_destroy(wsc_cls_grad *g) {
    if (!g) return;
    g->release();
    delete g;
}

int wsc_cls_grad_create(wsc_ctx *ctx, const wsc_net *net, const wsc_tensor_desc *weights, int n_weights, wsc_cls_grad **out) {
    WSC_CHECK(ctx && net && weights && out && n_weights > 0, WSC_ERR_INVALID, "wsc_cls_grad_create: null argument");
    WSC_TRY(need_cls("wsc_cls_grad_create", net));
    WSC_HIP(hipSetDevice(ctx->device));
    Dict d;
    WSC_TRY(descs_to_dict(weights, n_weights, &d));
    wsc_cls_grad *g = new wsc_cls_grad("wsc_cls_grad", ctx, net);
    // `<name>` as torch has it, [Cout][Cin][3][3] (Cin = 0: a vector [Cout]); the net's own tensor has that shape
    auto tensor = [&](const std::string &name, int Cout, int Cin, const HostTensor **t) -> int {
        auto it = d.find(name);
        WSC_CHECK(it != d.end() && it->second.data != nullptr, WSC_ERR_SHAPE, "layer '%s': missing", name.c_str());
        const HostTensor &w = it->second;
        const bool ok = Cin > 0 ? (w.ndim == 4 && w.shape[0] == Cout && w.shape[1] == Cin && w.shape[2] == 3 && w.shape[3] == 3)
                                : (w.ndim == 1 && w.shape[0] == Cout);
        WSC_CHECK(ok, WSC_ERR_SHAPE, "layer '%s': the net has it as [%d]%s, got ndim %d [%lld][%lld][%lld][%lld]", name.c_str(), Cout,
                  Cin > 0 ? ("[" + std::to_string(Cin) + "][3][3]").c_str() : "", w.ndim, (long long)w.shape[0], (long long)w.shape[1],
                  (long long)w.shape[2], (long long)w.shape[3]);
        *t = &w;
        return WSC_OK;
    };
    auto entry = [&](const std::string &name, int Cin, int Cout) {
        wsc_grad_entry e = {};
        std::strncpy(e.name, name.c_str(), sizeof(e.name) - 1);
        e.kh = e.kw = Cin > 0 ? 3 : 0;
        e.Cin = Cin; e.Cout = Cout;
        e.w_off = Cin > 0 ? g->grad_elems : -1;
        e.b_off = Cin > 0 ? -1 : g->grad_elems;
        g->layout.push_back(e);
        const long long at = g->grad_elems;
        g->grad_elems += Cin > 0 ? 9ll * Cin * Cout : Cout; // (no gaps: every float of the buffer is some parameter's)
        return at;
    };
    int widest = 64;
    auto build = [&]() -> int {
        g->op_layer.assign(net->ops.size(), -1);
        for (size_t i : trunk_conv_ops(net)) {
            const Op &op = net->ops[i];
            g->op_layer[i] = (int)g->layers.size();
            const ConvW &c = net->convs[op.conv];
            WSC_CHECK(c.kh == 3 && c.kw == 3 && c.stride == 1 && c.pad == 1 && c.dil == 1 && c.relu, WSC_ERR_INVALID,
                      "internal: layer '%s' is no 3 x 3 stride-1 SAME convolution with a ReLU", op.label.c_str());
            ClsGradLayer L;
            L.Cin = i == 0 ? 3 : c.Cin; L.Cout = c.Cout; L.bn = c.bn;
            const HostTensor *w, *b;
            WSC_TRY(tensor(op.label + ".weight", L.Cout, L.Cin, &w));
            WSC_TRY(tensor(op.label + ".bias", L.Cout, 0, &b));
            if (i > 0) { // OIHW -> HWIO -> the rotated kernel
                std::vector<float> hwio((size_t)9 * L.Cin * L.Cout), packed;
                for (int co = 0; co < L.Cout; ++co)
                    for (int ci = 0; ci < L.Cin; ++ci)
                        for (int t = 0; t < 9; ++t) hwio[((size_t)t * L.Cin + ci) * L.Cout + co] = w->data[((size_t)co * L.Cin + ci) * 9 + t];
                dgrad_pack(hwio.data(), 3, L.Cin, L.Cout, &packed);
                WSC_TRY(g->upload(packed, &L.w_rot));
                widest = std::max(widest, conv_cout_pad(L.Cin));
            }
            L.w_off = entry(op.label + ".weight", L.Cin, L.Cout);
            L.b_off = entry(op.label + ".bias", 0, L.Cout);
            if (L.bn >= 0) {
                const HostTensor *ga, *be;
                const std::string &bn = net->bns[L.bn].name;
                WSC_TRY(tensor(bn + ".weight", L.Cout, 0, &ga));
                WSC_TRY(tensor(bn + ".bias", L.Cout, 0, &be));
                L.g_off = entry(bn + ".weight", 0, L.Cout);
                L.be_off = entry(bn + ".bias", 0, L.Cout);
            }
            g->layers.push_back(L);
        }
        WSC_CHECK(net->cls_w && net->Ccls > 0 && net->F > 0, WSC_ERR_INVALID, "internal: a plain stack without its classifier");
        g->cls_w_off = g->grad_elems;
        g->cls_b_off = net->cls_b ? g->cls_w_off + (long long)net->Ccls * net->F : -1;
        g->param_elems = g->cls_w_off + (long long)net->Ccls * net->F + (net->cls_b ? net->Ccls : 0);
        return g->ones_zeros(widest);
    };
    const int st = build();
    if (st != WSC_OK) {
        wsc_cls_grad_destroy(g);
        return st;
    }
    *out = g;
    return WSC_OK;
}

int wsc_cls_grad_layout(const wsc_cls_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *grad_elems_out) {
    WSC_CHECK(g && n_out && grad_elems_out && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_cls_grad_layout: null argument");
    *n_out = (int)g->layout.size();
    *grad_elems_out = g->grad_elems;
    for (int i = 0; i < max_entries && i < (int)g->layout.size(); ++i) entries_out[i] = g->layout[i];
    return WSC_OK;
}

namespace {
// wsc_net_backward_cls (drop null) and wsc_net_backward_cls_drop (drop null at drop_prob = 0: the same launches)
int cls_backward(const char *fn, wsc_ctx *ctx, wsc_cls_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                 const float *dfeat_dev, const long long *dfeat_elems, float *grad_dev, long long grad_elems, const ClsDrop *drop) {
    WSC_TRY(grad_check(fn, ctx, g, grad_elems, tape_dev && dfeat_dev && grad_dev));
    WSC_TRY(cls_shape_check(fn, B, H, W, tape_dev));
    WSC_CHECK(((uintptr_t)dfeat_dev & 15) == 0 && ((uintptr_t)grad_dev & 15) == 0, WSC_ERR_INVALID, "%s: dfeat_dev / grad_dev must be 16-byte aligned", fn);
    const wsc_net *net = g->net;
    ClsTapePlan tp;
    WSC_TRY(cls_tape_plan(net, B, H, W, &tp));
    WSC_TRY(tape_check(fn, "wsc_net_cls_tape_plan", tape_elems, tp.t));
    int h_in, w_in;
    WSC_TRY(cls_feat_dims(fn, net, tp.pl, drop != nullptr, &h_in, &w_in));
    WSC_CHECK(!dfeat_elems || *dfeat_elems == (long long)B * h_in * w_in * net->F, WSC_ERR_INVALID,
              "%s: dfeat_elems = %lld, the map is [%d][%d][%d][%d] (wsc_net_cls_feat_dims)", fn, dfeat_elems ? *dfeat_elems : 0ll, B, h_in, w_in, net->F);
    const bool m7_site = drop && net->cls_max;
    PoolGeom branch;
    if (m7_site) WSC_TRY(cls_branch_pool(fn, net, tp.pl.hf, tp.pl.wf, &branch));
    // every layer's plan and the workspace they need, before anything is launched
    std::vector<WgradPlan> plans(g->layers.size());
    long long g_max = m7_site ? (long long)B * tp.pl.hf * tp.pl.wf * net->F : 0, dz_max = 0, slab_max = 0, part_max = 0;
    for (size_t i = 0; i < net->ops.size(); ++i) {
        const OpDims &d = tp.pl.ops[i];
        g_max = std::max(g_max, (long long)B * d.H * d.W * d.C);
        if (g->op_layer[i] < 0) continue;
        const size_t li = (size_t)g->op_layer[i];
        const ClsGradLayer &L = g->layers[li];
        WSC_TRY(wgrad_plan(ctx, B, d.Ho, d.Wo, L.Cin, L.Cout, 3, 1, 0, &plans[li]));
        const long long M = (long long)B * d.Ho * d.Wo;
        dz_max = std::max(dz_max, M * L.Cout);
        slab_max = std::max(slab_max, plans[li].slab_elems);
        part_max = std::max(part_max, (long long)relu_bias_grad_blocks(M) * L.Cout);
    }
    auto lines = LineCarver::lines;
    WSC_TRY(g->workspace(2 * lines(g_max) + 2 * lines(dz_max) + lines(slab_max) + lines(part_max)));
    LineCarver ws = {(char *)g->ws};
    float *gfree[2] = {ws.floats(g_max), ws.floats(g_max)};
    float *dbn = ws.floats(dz_max), *dz = ws.floats(dz_max), *slab = ws.floats(slab_max), *partial = ws.floats(part_max);
    auto at = [&](int entry) { return tape_dev + tp.t.off(entry); };

    const float *gcur = dfeat_dev; // the gradient of op i's output (behind its BatchNorm and its dropout site, where it has them)
    int nf = 0;
    if (m7_site) { // the site's own gradient (a dropped +0.0 that won the global max passes nothing on), then layer3_p2's
        const long long n = (long long)B * branch.Ho * branch.Wo * net->F;
        WSC_TRY(launch_seg_dropout_f32(ctx, dfeat_dev, gfree[0], nullptr, nullptr, n, 0ull, drop->drop_prob, drop->seed, drop->step, M7_DROP_SITE));
        WSC_TRY(launch_pool_grad(ctx, at(tp.out.back()), gfree[0], B, tp.pl.hf, tp.pl.wf, net->F, branch, gfree[1]));
        gcur = gfree[1];
    }
    for (int i = (int)net->ops.size() - 1; i >= 0; --i) {
        const Op &op = net->ops[i];
        const OpDims &d = tp.pl.ops[i];
        const float *x = at(i == 0 ? 0 : tp.out[i - 1]);
        float *gout = gfree[nf];
        if (op.type == OP_POOL) {
            PoolGeom pg;
            WSC_CHECK(pool_geom(op.rule, op.pk, op.ps, op.pp, op.avg, d.H, d.W, &pg), WSC_ERR_INVALID, "internal: a pool plan_dims let through");
            WSC_TRY(launch_pool_grad(ctx, x, gcur, B, d.H, d.W, d.C, pg, gout));
        } else {
            const size_t li = (size_t)g->op_layer[i];
            const ClsGradLayer &L = g->layers[li];
            const long long M = (long long)B * d.Ho * d.Wo;
            const float *a = at(tp.a[i]);
            const bool site = drop && op.drop_site >= 0;
            if (L.bn >= 0) {
                if (site) // (the mask regenerated from the counter: a kept BatchNorm output may be negative or 0.0)
                    WSC_TRY(launch_batch_norm_grad_drop(ctx, a, at(tp.stats[i]), net->bns[L.bn].gamma, gcur, M, L.Cout, dbn, grad_dev + L.g_off,
                                                        grad_dev + L.be_off, drop->drop_prob, drop->seed, drop->step, (unsigned)op.drop_site));
                else
                    WSC_TRY(launch_batch_norm_grad(ctx, a, at(tp.stats[i]), net->bns[L.bn].gamma, gcur, M, L.Cout, dbn, grad_dev + L.g_off,
                                                   grad_dev + L.be_off));
                gcur = dbn;
            }
            // (a site without BatchNorm: the taped post-ReLU value is > 0 exactly where kept and positive, as behind fc6 / fc7)
            const float relu_scale = site && L.bn < 0 ? seg_dropout_scale(drop->drop_prob) : 1.0f;
            WSC_TRY(launch_relu_bias_grad(ctx, a, gcur, M, L.Cout, relu_scale, dz, partial, grad_dev + L.b_off));
            WSC_TRY(wgrad_launch(ctx, plans[li], x, dz, d.Ho, d.Wo, L.Cin, L.Cout, 3, 1, slab, grad_dev + L.w_off));
            if (i > 0) WSC_TRY(dgrad_launch(ctx, dz, L.w_rot, g->ones, g->zeros, B, d.Ho, d.Wo, L.Cin, L.Cout, 3, 1, nullptr, gout));
        }
        gcur = gout;
        nf ^= 1;
    }
    return WSC_OK;
}
} // namespace

int wsc_net_backward_cls(wsc_ctx *ctx, wsc_cls_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                         const float *dfeat_dev, float *grad_dev, long long grad_elems) {
    return cls_backward("wsc_net_backward_cls", ctx, g, B, H, W, tape_dev, tape_elems, dfeat_dev, nullptr, grad_dev, grad_elems, nullptr);
}

int wsc_net_backward_cls_drop(wsc_ctx *ctx, wsc_cls_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                              const float *dfeat_dev, float *grad_dev, long long grad_elems, long long dfeat_elems, float drop_prob,
                              unsigned long long seed, long long step) {
    const char *fn = "wsc_net_backward_cls_drop";
    WSC_TRY(seg_dropout_check(fn, drop_prob, step));
    const ClsDrop drop = {drop_prob, seed, (unsigned)step};
    return cls_backward(fn, ctx, g, B, H, W, tape_dev, tape_elems, dfeat_dev, &dfeat_elems, grad_dev, grad_elems, drop_prob > 0.f ? &drop : nullptr);
}

// ---- the update half of a 01_train step (Keras' SGD with Nesterov momentum, 01_train/demo.py:60) and the repack of the updated
// parameters into the net; kernels: sgd.hip (the step), repack.hip ------------------------------------------------------
int wsc_cls_param_layout(const wsc_cls_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *param_elems_out) {
    WSC_CHECK(g && n_out && param_elems_out && max_entries >= 0 && (entries_out != nullptr || max_entries == 0), WSC_ERR_INVALID,
              "wsc_cls_param_layout: null argument");
    const wsc_net *net = g->net;
    const int n_grad = (int)g->layout.size();
    *n_out = n_grad + (g->cls_b_off >= 0 ? 2 : 1);
    *param_elems_out = g->param_elems;
    const std::string root = net->arch == WSC_ARCH_VGG16_CAM ? "vgg16" : "m7";
    for (int i = 0; i < max_entries && i < *n_out; ++i) {
        if (i < n_grad) {
            entries_out[i] = g->layout[i];
            continue;
        }
        wsc_grad_entry e = {};
        const bool w = i == n_grad;
        std::strncpy(e.name, (root + (w ? ".classifier.0.weight" : ".classifier.0.bias")).c_str(), sizeof(e.name) - 1);
        e.kh = e.kw = w ? 1 : 0;
        e.Cin = w ? net->F : 0; e.Cout = net->Ccls;
        e.w_off = w ? g->cls_w_off : -1;
        e.b_off = w ? -1 : g->cls_b_off;
        entries_out[i] = e;
    }
    return WSC_OK;
}

int wsc_cls_sgd_step(wsc_ctx *ctx, wsc_cls_grad *g, float *param_dev, const float *grad_dev, float *mom_dev, long long elems, float lr,
                     float momentum, int nesterov) {
    const char *fn = "wsc_cls_sgd_step";
    WSC_TRY(grad_check(fn, ctx, g, elems, param_dev && grad_dev && mom_dev, g ? g->param_elems : 0));
    WSC_CHECK(std::isfinite(lr) && lr >= 0.f, WSC_ERR_INVALID, "%s: lr = %g (finite, >= 0)", fn, (double)lr);
    WSC_CHECK(momentum >= 0.f && momentum < 1.f, WSC_ERR_INVALID, "%s: momentum = %g (0 <= momentum < 1)", fn, (double)momentum);
    WSC_CHECK(nesterov == 0 || nesterov == 1, WSC_ERR_INVALID, "%s: nesterov = %d (0 / 1)", fn, nesterov);
    WSC_CHECK((((uintptr_t)param_dev | (uintptr_t)grad_dev | (uintptr_t)mom_dev) & 3) == 0, WSC_ERR_INVALID, "%s: a buffer is not 4-byte aligned", fn);
    WSC_HIP(hipSetDevice(ctx->device));
    return cls_sgd_launch(ctx, param_dev, grad_dev, mom_dev, elems, lr, momentum, nesterov);
}

int wsc_net_cls_load_params(wsc_ctx *ctx, wsc_net *net, wsc_cls_grad *g, const float *param_dev, long long elems, const float *run_dev) {
    const char *fn = "wsc_net_cls_load_params";
    WSC_CHECK(ctx && net && g && param_dev, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_TRY(need_cls(fn, net));
    WSC_CHECK(g->net == net, WSC_ERR_INVALID, "%s: the wsc_cls_grad was created for another net", fn);
    WSC_TRY(grad_check(fn, ctx, g, elems, true, g->param_elems));
    // VGG16's head is the Linear itself unless the net was given a Grad-CAM alpha in its place; M7's head is always its
    // `gradcam_weights` tensor, which is no parameter of the training layout and stays as it is
    WSC_CHECK(net->arch != WSC_ARCH_VGG16_CAM || net->head_is_cls, WSC_ERR_INVALID,
              "%s: the net was built with `gradcam_weights`: its CAM head is not the classifier the parameters hold", fn);
    WSC_CHECK(((uintptr_t)param_dev & 3) == 0 && ((uintptr_t)run_dev & 3) == 0, WSC_ERR_INVALID, "%s: a buffer is not 4-byte aligned", fn);
    std::vector<ConvW *> convs;
    for (size_t i : trunk_conv_ops(net)) convs.push_back(&net->convs[net->ops[i].conv]);
    WSC_CHECK(convs.size() == g->layers.size(), WSC_ERR_INVALID, "internal: %d layers of the net, %d of the layout", (int)convs.size(),
              (int)g->layers.size());
    for (size_t i = 0; i < convs.size(); ++i) {
        const ConvW &c = *convs[i];
        const ClsGradLayer &L = g->layers[i];
        WSC_CHECK(conv_is_layer(c, 3, L.Cin, L.Cout) && c.bn == L.bn && (c.bn >= 0) == (c.s2 != nullptr && c.b2 != nullptr), WSC_ERR_INVALID,
                  "internal: layer %d of the layout is not the net's", (int)i);
    }
    WSC_HIP(hipSetDevice(ctx->device));
    const int C = net->Ccls, F = net->F;
    if (!g->repack.jobs_dev) { // the job tables: once per wsc_cls_grad (the packed buffers of both objects never move)
        std::vector<RepackJob> jobs;
        JobTable<VecCopyJob> vecs;
        JobTable<BnFoldJob> folds;
        long long run_off = 0;
        for (size_t i = 0; i < convs.size(); ++i) {
            const ConvW &c = *convs[i];
            const ClsGradLayer &L = g->layers[i];
            jobs.push_back(conv_repack_job(c, 3, L.Cin, L.Cout, L.w_off, L.b_off, L.w_rot));
            if (L.bn < 0) continue;
            const PlainBn &pb = net->bns[L.bn];
            add_vec(vecs, L.g_off, L.Cout, pb.gamma);
            add_vec(vecs, L.be_off, L.Cout, pb.beta);
            folds.add({L.g_off, L.be_off, run_off, L.Cout, 0, pb.eps_fold, c.s2, c.b2}, L.Cout, BN_FOLD_PER_BLOCK);
            run_off += 2ll * L.Cout;
        }
        add_vec(vecs, g->cls_w_off, C * F, net->cls_w);
        if (g->cls_b_off >= 0) add_vec(vecs, g->cls_b_off, C, net->cls_b);
        // (the conv table last: jobs_dev, what marks the tables as built, is set by its plan)
        WSC_TRY(vecs.upload(g));
        WSC_TRY(folds.upload(g));
        g->vecs = vecs;
        g->folds = folds;
        if (net->head_is_cls) { // the head: a 1 x 1 layer [F][C] without a bias, read from the transposed copy
            const ConvW &h = net->head;
            WSC_CHECK(h.kh == 1 && h.kw == 1 && h.form == CONV_FORM_GENERIC && h.Cin == F && h.Cout == C && !h.s2, WSC_ERR_INVALID,
                      "internal: the CAM head is no 1 x 1 layer over the %d feature channels", F);
            WSC_TRY(g->own((size_t)C * F * sizeof(float), (void **)&g->head_t));
            std::vector<RepackJob> hj(1, conv_repack_job(h, 1, F, C, 0, -1, nullptr));
            WSC_TRY(g->plan_repack(hj, &g->head_repack));
        }
        WSC_TRY(g->plan_repack(jobs));
    }
    WSC_TRY(repack_launch(ctx, g->repack, param_dev));
    WSC_TRY(vec_copy_launch(ctx, g->vecs.dev, g->vecs.n, g->vecs.blocks, param_dev));
    if (run_dev) WSC_TRY(bn_fold_launch(ctx, g->folds.dev, g->folds.n, g->folds.blocks, param_dev, run_dev));
    if (net->head_is_cls) {
        // (wsc_ctx_scratch_fill: the transposed copy is scratch of this call, kept by the object between calls)
        if (ctx->scratch_fill >= 0) WSC_HIP(hipMemsetAsync(g->head_t, ctx->scratch_fill, (size_t)C * F * sizeof(float), ctx->stream));
        WSC_TRY(transpose_cf_launch(ctx, param_dev + g->cls_w_off, C, F, g->head_t));
        WSC_TRY(repack_launch(ctx, g->head_repack, g->head_t));
    }
    return WSC_OK;
}

} // extern "C"
