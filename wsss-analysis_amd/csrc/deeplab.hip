// deeplab.hip -- the kernels around the conv stack of the SEC / DSRG DeepLab-VGG16 forward pass (03a_sec-dsrg):
//   fc8-softmax                build_sp_softmax (DSRG.py:297-300, SEC.py:246-249): a softmax, + min_prob, renormalised
//   tf.image.resize_bilinear   TensorFlow 1.x, align_corners=False -- the legacy sampler WITHOUT the half-pixel offset
//                              (rescale_output DSRG.py:450, the CRF layer's zoom :319-321, image_preprocess model.py:335)
//   NHWC float32 [N][H][W][3] -> the NHWC4 activation the first conv layer reads
// All of them are HBM-bound maps: one thread per output vector, no LDS.  (The nets' pools: pool.hip.)
#include "common.h"
#include "tf_resize.h"

#include <cmath>

namespace {

// float32 NHWC [N][H][W][3] (what the reference feeds net["input"]: BGR minus mean) -> NHWC4 activation, 4th channel zero.
// IEEE-half planes: a value the saturating conversion cuts (|v| >= 65504, NaN) raises the ctx's range flag like a conv epilogue
// does -- the planes then do not hold the reference's input.  bfloat16 and fp32 planes: NaN and +-inf raise it (a whole net is
// loud in every precision; misc_kernels.hip's packs have the same test).
__global__ __launch_bounds__(256) void nhwc3_to_nhwc4_kernel(const float *__restrict__ x, long long npix, bf16_t *__restrict__ y,
                                                             bf16_t *__restrict__ y_lo, int fmt, unsigned *range) {
    bool ovf = false;
    const float lim = fmt == 1 ? 65504.f : INFINITY;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const float c0 = x[3 * i], c1 = x[3 * i + 1], c2 = x[3 * i + 2];
        const bf16_t h0 = f32_to_h16(c0, fmt), h1 = f32_to_h16(c1, fmt), h2 = f32_to_h16(c2, fmt);
        ovf = ovf || !(fabsf(c0) < lim) || !(fabsf(c1) < lim) || !(fabsf(c2) < lim);
        reinterpret_cast<uint2 *>(y)[i] = make_uint2((uint32_t)h0 | ((uint32_t)h1 << 16), (uint32_t)h2);
        if (y_lo != nullptr) {
            const bf16_t l0 = f32_to_h16(c0 - h16_to_f32(h0, fmt), fmt), l1 = f32_to_h16(c1 - h16_to_f32(h1, fmt), fmt),
                         l2 = f32_to_h16(c2 - h16_to_f32(h2, fmt), fmt);
            reinterpret_cast<uint2 *>(y_lo)[i] = make_uint2((uint32_t)l0 | ((uint32_t)l1 << 16), (uint32_t)l2);
        }
    }
    if (ovf) *range = 3u;
}
__global__ __launch_bounds__(256) void nhwc3_to_nhwc4_f32_kernel(const float *__restrict__ x, long long npix, f32x4_t *__restrict__ y,
                                                                 unsigned *range) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const float c0 = x[3 * i], c1 = x[3 * i + 1], c2 = x[3 * i + 2];
        bad = bad || !(fabsf(c0) < INFINITY) || !(fabsf(c1) < INFINITY) || !(fabsf(c2) < INFINITY);
        y[i] = f32x4_t{c0, c1, c2, 0.f};
    }
    if (bad) *range = 3u;
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

int launch_nhwc3_to_nhwc4(wsc_ctx *ctx, const float *x, int N, int H, int W, Act y) {
    const long long npix = (long long)N * H * W;
    const bool f32 = y.is_f32();
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)npix * (12 + (f32 ? 16 : (y.lo ? 16 : 8))));
    if (f32) hipLaunchKernelGGL(nhwc3_to_nhwc4_f32_kernel, dim3(wsc_grid_for(npix)), dim3(256), 0, ctx->stream, x, npix, (f32x4_t *)y.f32(),
                              ctx->range_dev);
    else
        hipLaunchKernelGGL(nhwc3_to_nhwc4_kernel, dim3(wsc_grid_for(npix)), dim3(256), 0, ctx->stream, x, npix, y.h16(), y.h16_lo(), y.fmt(),
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
    hipLaunchKernelGGL(fc8_softmax_kernel, dim3(wsc_grid_for(M)), dim3(256), 0, ctx->stream, s, M, C, min_prob, fc8, prob);
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
    hipLaunchKernelGGL(resize_bilinear_tf_kernel, dim3(wsc_grid_for(total)), dim3(256), 0, ctx->stream, src_dev, B, h, w, C, dst_dev, H, W,
                       (float)h / (float)H, (float)w / (float)W);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int wsc_fc8_softmax(wsc_ctx *ctx, const float *const *fc8_dev, int n_in, long long M, int C, float min_prob, float *sum_dev,
                    float *prob_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_fc8_softmax: null ctx");
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_fc8_softmax(ctx, fc8_dev, n_in, M, C, min_prob, sum_dev, prob_dev);
}

} // extern "C"
