// deeplab.hip -- the kernels around the conv stack of the SEC / DSRG DeepLab-VGG16 forward pass (03a_sec-dsrg):
//   TF-`SAME` 3x3 pooling      max_pool stride 2 / 1 and avg_pool stride 1 of build_block (DSRG.py:229-246, SEC.py:173-188)
//   TF / Keras MaxPooling2D    window 2 or 3, stride 1 or 2, `SAME` or `VALID`: the pools a Keras-side session's architecture
//                              file gives the CAM nets (02_cues/demo.py:104-124 model_from_json; the `pool_spec` of net.hip)
//   fc8-softmax                build_sp_softmax (DSRG.py:297-300, SEC.py:246-249): a softmax, + min_prob, renormalised
//   tf.image.resize_bilinear   TensorFlow 1.x, align_corners=False -- the legacy sampler WITHOUT the half-pixel offset
//                              (rescale_output DSRG.py:450, the CRF layer's zoom :319-321, image_preprocess model.py:335)
//   NHWC float32 [N][H][W][3] -> the NHWC4 activation the first conv layer reads
// All of them are HBM-bound maps with no reuse beyond a 3x3 footprint: one thread per output vector, no LDS.
//
// TF `SAME` per axis: out = ceil(in / stride), pad_total = max((out - 1) stride + 3 - in, 0), pad_before = pad_total / 2 (floor),
// the rest after: 1 / 1 on an odd size, 0 / 1 on an even size at stride 2 (which one symmetric `pad` cannot express).  Max
// ignores the padding (-inf, not 0); the average divides by the number of IN-IMAGE taps (4 at a corner, 6 on an edge).
// A window K in place of the 3 is the same rule (pool_tf_dims); TF `VALID`: out = floor((in - K) / stride) + 1, no padding.
#include "common.h"
#include "tf_resize.h"

#include <cmath>

namespace {

inline int grid_for(long long total, int block = 256, int cap = 256 * 16) {
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

struct PoolArgs {
    int N, H, W, C, Ho, Wo;
    int stride, pad_t, pad_l;
    int avg; // 0: max, 1: average over the in-image taps
};

// 16-bit planes (either format; the lo plane optional), 8 channels per thread.  A value is hi + lo, exact in fp32 (11 + 11 or
// 8 + 8 significant bits).  Max: the maximum of those values, split again -- the pair it came from.  Average: summed and
// divided in double (9 fp32 terms: exact but for the final rounding), then split.
__global__ __launch_bounds__(256) void pool_same_h16_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, PoolArgs a,
                                                            bf16_t *__restrict__ y, bf16_t *__restrict__ y_lo, int fmt) {
    const int C8 = a.C >> 3;
    const long long total = (long long)a.N * a.Ho * a.Wo * C8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        long long pix = i / C8;
        const int wo = (int)(pix % a.Wo);
        pix /= a.Wo;
        const int ho = (int)(pix % a.Ho);
        const int n = (int)(pix / a.Ho);
        float best[8];
        double sum[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            best[j] = -INFINITY;
            sum[j] = 0.0;
        }
        int cnt = 0;
        for (int dy = 0; dy < 3; ++dy) {
            const int hi = ho * a.stride - a.pad_t + dy;
            if ((unsigned)hi >= (unsigned)a.H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int wi = wo * a.stride - a.pad_l + dx;
                if ((unsigned)wi >= (unsigned)a.W) continue;
                const long long o = (((long long)n * a.H + hi) * a.W + wi) * a.C + c8 * 8;
                const uint4 v = *reinterpret_cast<const uint4 *>(x + o);
                const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
                float f[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f[2 * j] = h16_to_f32((bf16_t)(vw[j] & 0xffffu), fmt);
                    f[2 * j + 1] = h16_to_f32((bf16_t)(vw[j] >> 16), fmt);
                }
                if (x_lo != nullptr) {
                    const uint4 l = *reinterpret_cast<const uint4 *>(x_lo + o);
                    const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f[2 * j] += h16_to_f32((bf16_t)(lw[j] & 0xffffu), fmt);
                        f[2 * j + 1] += h16_to_f32((bf16_t)(lw[j] >> 16), fmt);
                    }
                }
                ++cnt;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    best[j] = fmaxf(best[j], f[j]);
                    sum[j] += (double)f[j];
                }
            }
        }
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a.avg ? (float)(sum[j] / (double)cnt) : best[j];
        uint32_t hw[4], lw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf16_t h0 = f32_to_h16(r[2 * j], fmt), h1 = f32_to_h16(r[2 * j + 1], fmt);
            hw[j] = (uint32_t)h0 | ((uint32_t)h1 << 16);
            const bf16_t l0 = f32_to_h16(r[2 * j] - h16_to_f32(h0, fmt), fmt);
            const bf16_t l1 = f32_to_h16(r[2 * j + 1] - h16_to_f32(h1, fmt), fmt);
            lw[j] = (uint32_t)l0 | ((uint32_t)l1 << 16);
        }
        const long long oo = (((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c8 * 8;
        *reinterpret_cast<uint4 *>(y + oo) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        if (y_lo != nullptr) *reinterpret_cast<uint4 *>(y_lo + oo) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    }
}

// WSC_PREC_F32: one plane of fp32, 4 channels per thread; max is bit-exact, the average is the double sum rounded once
__global__ __launch_bounds__(256) void pool_same_f32_kernel(const float *__restrict__ x, PoolArgs a, float *__restrict__ y) {
    const int C4 = a.C >> 2;
    const long long total = (long long)a.N * a.Ho * a.Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long pix = i / C4;
        const int wo = (int)(pix % a.Wo);
        pix /= a.Wo;
        const int ho = (int)(pix % a.Ho);
        const int n = (int)(pix / a.Ho);
        f32x4_t best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        int cnt = 0;
        for (int dy = 0; dy < 3; ++dy) {
            const int hi = ho * a.stride - a.pad_t + dy;
            if ((unsigned)hi >= (unsigned)a.H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int wi = wo * a.stride - a.pad_l + dx;
                if ((unsigned)wi >= (unsigned)a.W) continue;
                const f32x4_t v = *reinterpret_cast<const f32x4_t *>(x + ((((long long)n * a.H + hi) * a.W + wi) * a.C + c4 * 4));
                ++cnt;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    best[j] = fmaxf(best[j], v[j]);
                    sum[j] += (double)v[j];
                }
            }
        }
        f32x4_t r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = a.avg ? (float)(sum[j] / (double)cnt) : best[j];
        *reinterpret_cast<f32x4_t *>(y + ((((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c4 * 4)) = r;
    }
}

// ---- TF / Keras MaxPooling2D: window K x K (compile time, taps unrolled), stride 1 / 2, SAME or VALID (pool_tf_dims) ------------
struct PoolTfArgs {
    int N, H, W, C, Ho, Wo;
    int stride, pad_t, pad_l; // VALID: both pads 0, every tap in the image
};

// 16-bit planes (either format; the lo plane optional), 8 channels per thread: pool_same_h16_kernel's maximum -- of the fp32
// values hi + lo, split again
template <int K>
__global__ __launch_bounds__(256) void pool_tf_h16_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, PoolTfArgs a,
                                                          bf16_t *__restrict__ y, bf16_t *__restrict__ y_lo, int fmt) {
    const int C8 = a.C >> 3;
    const long long total = (long long)a.N * a.Ho * a.Wo * C8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        long long pix = i / C8;
        const int wo = (int)(pix % a.Wo);
        pix /= a.Wo;
        const int ho = (int)(pix % a.Ho);
        const int n = (int)(pix / a.Ho);
        float best[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < K; ++dy) {
            const int hi = ho * a.stride - a.pad_t + dy;
            if ((unsigned)hi >= (unsigned)a.H) continue;
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                const int wi = wo * a.stride - a.pad_l + dx;
                if ((unsigned)wi >= (unsigned)a.W) continue;
                const long long o = (((long long)n * a.H + hi) * a.W + wi) * a.C + c8 * 8;
                const uint4 v = *reinterpret_cast<const uint4 *>(x + o);
                const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
                float f[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f[2 * j] = h16_to_f32((bf16_t)(vw[j] & 0xffffu), fmt);
                    f[2 * j + 1] = h16_to_f32((bf16_t)(vw[j] >> 16), fmt);
                }
                if (x_lo != nullptr) {
                    const uint4 l = *reinterpret_cast<const uint4 *>(x_lo + o);
                    const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f[2 * j] += h16_to_f32((bf16_t)(lw[j] & 0xffffu), fmt);
                        f[2 * j + 1] += h16_to_f32((bf16_t)(lw[j] >> 16), fmt);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) best[j] = fmaxf(best[j], f[j]);
            }
        }
        uint32_t hw[4], lw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf16_t h0 = f32_to_h16(best[2 * j], fmt), h1 = f32_to_h16(best[2 * j + 1], fmt);
            hw[j] = (uint32_t)h0 | ((uint32_t)h1 << 16);
            const bf16_t l0 = f32_to_h16(best[2 * j] - h16_to_f32(h0, fmt), fmt);
            const bf16_t l1 = f32_to_h16(best[2 * j + 1] - h16_to_f32(h1, fmt), fmt);
            lw[j] = (uint32_t)l0 | ((uint32_t)l1 << 16);
        }
        const long long oo = (((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c8 * 8;
        *reinterpret_cast<uint4 *>(y + oo) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        if (y_lo != nullptr) *reinterpret_cast<uint4 *>(y_lo + oo) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    }
}

// WSC_PREC_F32: one plane of fp32, 4 channels per thread, bit-exact
template <int K>
__global__ __launch_bounds__(256) void pool_tf_f32_kernel(const float *__restrict__ x, PoolTfArgs a, float *__restrict__ y) {
    const int C4 = a.C >> 2;
    const long long total = (long long)a.N * a.Ho * a.Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long pix = i / C4;
        const int wo = (int)(pix % a.Wo);
        pix /= a.Wo;
        const int ho = (int)(pix % a.Ho);
        const int n = (int)(pix / a.Ho);
        f32x4_t best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int dy = 0; dy < K; ++dy) {
            const int hi = ho * a.stride - a.pad_t + dy;
            if ((unsigned)hi >= (unsigned)a.H) continue;
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                const int wi = wo * a.stride - a.pad_l + dx;
                if ((unsigned)wi >= (unsigned)a.W) continue;
                const f32x4_t v = *reinterpret_cast<const f32x4_t *>(x + ((((long long)n * a.H + hi) * a.W + wi) * a.C + c4 * 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) best[j] = fmaxf(best[j], v[j]);
            }
        }
        *reinterpret_cast<f32x4_t *>(y + ((((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c4 * 4)) = best;
    }
}

// float32 NHWC [N][H][W][3] (what the reference feeds net["input"]: BGR minus mean) -> NHWC4 activation, 4th channel zero.
// IEEE-half planes: a value the saturating conversion cuts (|v| >= 65504, NaN) raises the ctx's range flag like a conv epilogue
// does -- the planes then do not hold the reference's input.
__global__ __launch_bounds__(256) void nhwc3_to_nhwc4_kernel(const float *__restrict__ x, long long npix, bf16_t *__restrict__ y,
                                                             bf16_t *__restrict__ y_lo, int fmt, unsigned *range) {
    bool ovf = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const float c0 = x[3 * i], c1 = x[3 * i + 1], c2 = x[3 * i + 2];
        const bf16_t h0 = f32_to_h16(c0, fmt), h1 = f32_to_h16(c1, fmt), h2 = f32_to_h16(c2, fmt);
        if (fmt == 1) ovf = ovf || !(fabsf(c0) < 65504.f) || !(fabsf(c1) < 65504.f) || !(fabsf(c2) < 65504.f);
        reinterpret_cast<uint2 *>(y)[i] = make_uint2((uint32_t)h0 | ((uint32_t)h1 << 16), (uint32_t)h2);
        if (y_lo != nullptr) {
            const bf16_t l0 = f32_to_h16(c0 - h16_to_f32(h0, fmt), fmt), l1 = f32_to_h16(c1 - h16_to_f32(h1, fmt), fmt),
                         l2 = f32_to_h16(c2 - h16_to_f32(h2, fmt), fmt);
            reinterpret_cast<uint2 *>(y_lo)[i] = make_uint2((uint32_t)l0 | ((uint32_t)l1 << 16), (uint32_t)l2);
        }
    }
    if (ovf) *range = 3u;
}
__global__ __launch_bounds__(256) void nhwc3_to_nhwc4_f32_kernel(const float *__restrict__ x, long long npix, f32x4_t *__restrict__ y) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x)
        y[i] = f32x4_t{x[3 * i], x[3 * i + 1], x[3 * i + 2], 0.f};
}

// fc8-softmax of one pixel per thread, fp32: x = in[0] + in[1] + ... in that order (the ASPP branches; one input for SEC),
// e = exp(x - max), p = e / sum(e) + min_prob, p /= sum(p).  The rows ([C] floats) are read three times (L1 / L2 hits).
struct SoftmaxIn {
    const float *p[4];
    int n;
};
__global__ __launch_bounds__(256) void fc8_softmax_kernel(SoftmaxIn in, long long M, int C, float min_prob, float *__restrict__ fc8,
                                                          float *__restrict__ prob) {
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const long long o = m * C;
        auto logit = [&](int c) {
            float v = in.p[0][o + c];
            for (int k = 1; k < in.n; ++k) v += in.p[k][o + c];
            return v;
        };
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) {
            const float v = logit(c);
            if (fc8 != nullptr) fc8[o + c] = v;
            mx = fmaxf(mx, v);
        }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(logit(c) - mx);
        float sp = 0.f;
        for (int c = 0; c < C; ++c) sp += expf(logit(c) - mx) / se + min_prob;
        for (int c = 0; c < C; ++c) prob[o + c] = (expf(logit(c) - mx) / se + min_prob) / sp;
    }
}

// tf.image.resize_bilinear(align_corners=False) of TensorFlow 1.x on NHWC float32: tf_resize.h's rule and its lerp (this file is
// compiled without FMA contraction, as the header demands)
__global__ __launch_bounds__(256) void resize_bilinear_tf_kernel(const float *__restrict__ src, int B, int h, int w, int C,
                                                                 float *__restrict__ dst, int H, int W, float sy, float sx) {
    const long long total = (long long)B * H * W * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long pix = i / C;
        const int X = (int)(pix % W);
        pix /= W;
        const int Y = (int)(pix % H);
        const long long b = pix / H;
        // tf_tap of both axes, written out interleaved (two calls: the same values, another instruction schedule of this kernel)
        const float fy = (float)Y * sy, fx = (float)X * sx;
        const int y0 = min((int)floorf(fy), h - 1), x0 = min((int)floorf(fx), w - 1);
        const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
        const float ty = fy - (float)y0, tx = fx - (float)x0;
        const float *s = src + b * h * w * C + c;
        const float tl = s[((long long)y0 * w + x0) * C], tr = s[((long long)y0 * w + x1) * C];
        const float bl = s[((long long)y1 * w + x0) * C], br = s[((long long)y1 * w + x1) * C];
        dst[i] = tf_lerp(tl, tr, bl, br, tx, ty);
    }
}

} // namespace

void pool_same_dims(int in, int stride, int *out, int *pad_before) {
    const int o = (in + stride - 1) / stride;
    int pad_total = (o - 1) * stride + 3 - in;
    if (pad_total < 0) pad_total = 0;
    *out = o;
    *pad_before = pad_total / 2;
}

int launch_pool_same(wsc_ctx *ctx, Act x, int N, int H, int W, int C, int avg, int stride, Act y) {
    WSC_CHECK(x && y && y.prec == x.prec, WSC_ERR_INVALID, "pool (SAME): input and output of different precisions");
    WSC_CHECK(C > 0 && C % 8 == 0, WSC_ERR_INVALID, "pool (SAME): C=%d not a multiple of 8", C);
    WSC_CHECK(N > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2) && (!avg || stride == 1), WSC_ERR_INVALID,
              "pool (SAME): 3x3 max at stride 1 / 2 or 3x3 average at stride 1, got stride %d on %d x %d x %d", stride, N, H, W);
    PoolArgs a;
    a.N = N; a.H = H; a.W = W; a.C = C; a.stride = stride; a.avg = avg ? 1 : 0;
    pool_same_dims(H, stride, &a.Ho, &a.pad_t);
    pool_same_dims(W, stride, &a.Wo, &a.pad_l);
    const bool f32 = x.is_f32();
    const long long total = (long long)N * a.Ho * a.Wo * (C / (f32 ? 4 : 8));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, ((double)N * H * W * C + (double)N * a.Ho * a.Wo * C) * (f32 ? 4 : (x.lo ? 4 : 2)));
    if (f32) hipLaunchKernelGGL(pool_same_f32_kernel, dim3(grid_for(total)), dim3(256), 0, ctx->stream, x.f32(), a, y.f32());
    else
        hipLaunchKernelGGL(pool_same_h16_kernel, dim3(grid_for(total)), dim3(256), 0, ctx->stream, x.h16(), x.h16_lo(), a, y.h16(),
                           y.h16_lo(), x.fmt());
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

bool pool_tf_dims(int in, int k, int stride, int same, int *out, int *pad_before) {
    *pad_before = 0;
    if (same) {
        const int o = (in + stride - 1) / stride;
        int pad_total = (o - 1) * stride + k - in;
        if (pad_total < 0) pad_total = 0;
        *out = o;
        *pad_before = pad_total / 2;
        return in >= 1;
    }
    *out = in >= k ? (in - k) / stride + 1 : 0;
    return in >= k;
}

int launch_pool_tf(wsc_ctx *ctx, Act x, int N, int H, int W, int C, int k, int stride, int same, Act y) {
    WSC_CHECK(x && y && y.prec == x.prec, WSC_ERR_INVALID, "pool (TF): input and output of different precisions");
    WSC_CHECK(C > 0 && C % 8 == 0, WSC_ERR_INVALID, "pool (TF): C=%d not a multiple of 8", C);
    WSC_CHECK((k == 2 || k == 3) && (stride == 1 || stride == 2) && stride <= k && (same == 0 || same == 1), WSC_ERR_INVALID,
              "pool (TF): window 2 / 3, stride 1 / 2 (<= window), SAME 0 / 1; got window %d stride %d same %d", k, stride, same);
    PoolTfArgs a;
    a.N = N; a.H = H; a.W = W; a.C = C; a.stride = stride;
    WSC_CHECK(N > 0 && pool_tf_dims(H, k, stride, same, &a.Ho, &a.pad_t) && pool_tf_dims(W, k, stride, same, &a.Wo, &a.pad_l),
              WSC_ERR_INVALID, "pool (TF): %d x %d x %d is no input of a %d x %d %s window", N, H, W, k, k, same ? "SAME" : "VALID");
    const bool f32 = x.is_f32();
    const long long total = (long long)N * a.Ho * a.Wo * (C / (f32 ? 4 : 8));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, ((double)N * H * W * C + (double)N * a.Ho * a.Wo * C) * (f32 ? 4 : (x.lo ? 4 : 2)));
    const dim3 grid(grid_for(total)), block(256);
    if (f32) {
        if (k == 2) hipLaunchKernelGGL(pool_tf_f32_kernel<2>, grid, block, 0, ctx->stream, x.f32(), a, y.f32());
        else hipLaunchKernelGGL(pool_tf_f32_kernel<3>, grid, block, 0, ctx->stream, x.f32(), a, y.f32());
    } else if (k == 2) {
        hipLaunchKernelGGL(pool_tf_h16_kernel<2>, grid, block, 0, ctx->stream, x.h16(), x.h16_lo(), a, y.h16(), y.h16_lo(), x.fmt());
    } else {
        hipLaunchKernelGGL(pool_tf_h16_kernel<3>, grid, block, 0, ctx->stream, x.h16(), x.h16_lo(), a, y.h16(), y.h16_lo(), x.fmt());
    }
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_nhwc3_to_nhwc4(wsc_ctx *ctx, const float *x, int N, int H, int W, Act y) {
    const long long npix = (long long)N * H * W;
    const bool f32 = y.is_f32();
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)npix * (12 + (f32 ? 16 : (y.lo ? 16 : 8))));
    if (f32) hipLaunchKernelGGL(nhwc3_to_nhwc4_f32_kernel, dim3(grid_for(npix)), dim3(256), 0, ctx->stream, x, npix, (f32x4_t *)y.f32());
    else
        hipLaunchKernelGGL(nhwc3_to_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, ctx->stream, x, npix, y.h16(), y.h16_lo(), y.fmt(),
                           ctx->range_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_fc8_softmax(wsc_ctx *ctx, const float *const *in, int n_in, long long M, int C, float min_prob, float *fc8, float *prob) {
    WSC_CHECK(in && n_in >= 1 && n_in <= 4 && prob, WSC_ERR_INVALID, "fc8-softmax: 1 .. 4 inputs and an output, got %d", n_in);
    WSC_CHECK(C >= 1 && M >= 0 && min_prob >= 0.f, WSC_ERR_INVALID, "fc8-softmax: C=%d, min_prob=%g", C, (double)min_prob);
    SoftmaxIn s = {};
    s.n = n_in;
    for (int k = 0; k < n_in; ++k) {
        WSC_CHECK(in[k] != nullptr, WSC_ERR_INVALID, "fc8-softmax: input %d is null", k);
        s.p[k] = in[k];
    }
    if (M == 0) return WSC_OK;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)M * C * 4 * (n_in + 1 + (fc8 ? 1 : 0)));
    hipLaunchKernelGGL(fc8_softmax_kernel, dim3(grid_for(M)), dim3(256), 0, ctx->stream, s, M, C, min_prob, fc8, prob);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

extern "C" {

int wsc_resize_bilinear_tf(wsc_ctx *ctx, const float *src_dev, int B, int h, int w, int C, float *dst_dev, int H, int W) {
    WSC_CHECK(ctx && src_dev && dst_dev, WSC_ERR_INVALID, "wsc_resize_bilinear_tf: null argument");
    WSC_CHECK(B >= 1 && h >= 1 && w >= 1 && C >= 1 && H >= 1 && W >= 1, WSC_ERR_INVALID,
              "wsc_resize_bilinear_tf: B=%d, %d x %d x %d -> %d x %d", B, h, w, C, H, W);
    WSC_HIP(hipSetDevice(ctx->device));
    const long long total = (long long)B * H * W * C;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)total * 4 + (double)B * h * w * C * 4);
    hipLaunchKernelGGL(resize_bilinear_tf_kernel, dim3(grid_for(total)), dim3(256), 0, ctx->stream, src_dev, B, h, w, C, dst_dev, H, W,
                       (float)h / (float)H, (float)w / (float)W);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int wsc_pool_same_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int avg, int stride, int precision, float *y_dev) {
    WSC_CHECK(ctx && x_dev && y_dev, WSC_ERR_INVALID, "wsc_pool_same_nhwc: null argument");
    WSC_CHECK(precision >= WSC_PREC_BF16 && precision <= WSC_PREC_F32, WSC_ERR_INVALID, "unknown precision %d", precision);
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && (stride == 1 || stride == 2), WSC_ERR_INVALID,
              "wsc_pool_same_nhwc: %d x %d x %d x %d, stride %d", N, H, W, C, stride);
    WSC_HIP(hipSetDevice(ctx->device));
    const wsc_precision prec = (wsc_precision)precision;
    int Ho, Wo, pt, pl;
    pool_same_dims(H, stride, &Ho, &pt);
    pool_same_dims(W, stride, &Wo, &pl);
    const size_t in_e = (size_t)N * H * W * C, out_e = (size_t)N * Ho * Wo * C;
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, act_bytes(in_e, prec) + act_bytes(out_e, prec), &ws));
    char *p = (char *)ws;
    const Act xi = act_carve(p, in_e, prec), yo = act_carve(p, out_e, prec);
    // (the layout change of the single-layer entry with one "pixel" per sample row: NHWC stays NHWC, the values take the planes)
    WSC_TRY(launch_nchw_to_nhwc(ctx, x_dev, N * H * W, C, 1, xi));
    WSC_TRY(launch_pool_same(ctx, xi, N, H, W, C, avg, stride, yo));
    return launch_act_to_f32(ctx, yo, out_e, y_dev);
}

int wsc_pool_tf_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int k, int stride, int same, int precision,
                     float *y_dev) {
    WSC_CHECK(ctx && x_dev && y_dev, WSC_ERR_INVALID, "wsc_pool_tf_nhwc: null argument");
    WSC_CHECK(precision >= WSC_PREC_BF16 && precision <= WSC_PREC_F32, WSC_ERR_INVALID, "unknown precision %d", precision);
    WSC_CHECK((k == 2 || k == 3) && (stride == 1 || stride == 2) && stride <= k && (same == 0 || same == 1), WSC_ERR_INVALID,
              "wsc_pool_tf_nhwc: window %d stride %d same %d (window 2 / 3, stride 1 / 2, same 0 / 1)", k, stride, same);
    int Ho = 0, Wo = 0, pt, pl;
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && pool_tf_dims(H, k, stride, same, &Ho, &pt) && pool_tf_dims(W, k, stride, same, &Wo, &pl),
              WSC_ERR_INVALID, "wsc_pool_tf_nhwc: %d x %d x %d x %d is no input of a %d x %d %s window", N, H, W, C, k, k,
              same ? "SAME" : "VALID");
    WSC_HIP(hipSetDevice(ctx->device));
    const wsc_precision prec = (wsc_precision)precision;
    const size_t in_e = (size_t)N * H * W * C, out_e = (size_t)N * Ho * Wo * C;
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, act_bytes(in_e, prec) + act_bytes(out_e, prec), &ws));
    char *p = (char *)ws;
    const Act xi = act_carve(p, in_e, prec), yo = act_carve(p, out_e, prec);
    WSC_TRY(launch_nchw_to_nhwc(ctx, x_dev, N * H * W, C, 1, xi)); // (NHWC stays NHWC: wsc_pool_same_nhwc)
    WSC_TRY(launch_pool_tf(ctx, xi, N, H, W, C, k, stride, same, yo));
    return launch_act_to_f32(ctx, yo, out_e, y_dev);
}

int wsc_fc8_softmax(wsc_ctx *ctx, const float *const *fc8_dev, int n_in, long long M, int C, float min_prob, float *sum_dev,
                    float *prob_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_fc8_softmax: null ctx");
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_fc8_softmax(ctx, fc8_dev, n_in, M, C, min_prob, sum_dev, prob_dev);
}

} // extern "C"
