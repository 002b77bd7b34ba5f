// seg_chain.hip -- the steps between the device-resident pieces of the SEC / DSRG prediction loop (03a_sec-dsrg) that the host
// stood in for:
//   seg_preprocess_u8_kernel   image_preprocess of the evaluation phases (model.py:332-346) for a ragged batch of decoded uint8
//                              RGB images: TF 1.x resize_bilinear(align_corners=False) of float(u8), RGB -> BGR, minus the mean
//   seg_crf_image_u8_kernel    the CRF layer's zoomed image (DSRG.py:318-319,325 / SEC.py build_crf): x + mean, TF resize to the
//                              seed size, image.astype(np.uint8)
//   seg_crf_logprob_kernel     the tail of the `crf` closure (DSRG.py:329-332): clamp at min_prob, renormalise over the classes,
//                              log; class-major marginals in, NHWC out
//   seg_planes_from_nhwc_kernel  NHWC maps -> class-major planes (what wsc_seg_resize_argmax reads): the is_eval=False pass
// One thread per output pixel, grid-stride; every kernel moves each byte once and has no reuse: no LDS.
//
// The TF sampler is tf_resize.h's, the one wsc_resize_bilinear_tf runs: a value has the bits that entry point gives for it (this
// file is compiled without FMA contraction, as the header demands).
#include "common.h"
#include "tf_resize.h"

#include <limits.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

struct PreJob {
    long long src_off; // byte offset of the image's [h][w][3] block
    int h, w;
};
struct Mean3 {
    float v[3];
};

// img: packed uint8 RGB blocks; x: [n][H][W][3], x[..][c] = resized[..][2 - c] - mean[c]
__global__ __launch_bounds__(256) void seg_preprocess_u8_kernel(const uint8_t *__restrict__ img, const PreJob *__restrict__ jobs, Mean3 mean,
                                                                int H, int W, float *__restrict__ x) {
    const PreJob job = jobs[blockIdx.y];
    const long long n = (long long)H * W;
    const float sy = (float)job.h / (float)H, sx = (float)job.w / (float)W;
    const uint8_t *src = img + job.src_off;
    float *dst = x + (long long)blockIdx.y * n * 3;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int Y = (int)(p / W), X = (int)(p - (long long)Y * W);
        int y0, y1, x0, x1;
        float ty, tx;
        tf_tap(Y, sy, job.h, y0, y1, ty);
        tf_tap(X, sx, job.w, x0, x1, tx);
        const uint8_t *tl = src + ((long long)y0 * job.w + x0) * 3, *tr = src + ((long long)y0 * job.w + x1) * 3;
        const uint8_t *bl = src + ((long long)y1 * job.w + x0) * 3, *br = src + ((long long)y1 * job.w + x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = 2 - c;
            dst[p * 3 + c] = tf_lerp((float)tl[s], (float)tr[s], (float)bl[s], (float)br[s], tx, ty) - mean.v[c];
        }
    }
}

// x: [B][H][W][3]; out: uint8 [B][sh][sw][3] = (uint8_t)(int32_t) resize(x + mean)
__global__ __launch_bounds__(256) void seg_crf_image_u8_kernel(const float *__restrict__ x, int H, int W, Mean3 mean, int sh, int sw,
                                                               uint8_t *__restrict__ out) {
    const long long n = (long long)sh * sw;
    const float sy = (float)H / (float)sh, sx = (float)W / (float)sw;
    const float *src = x + (long long)blockIdx.y * H * W * 3;
    uint8_t *dst = out + (long long)blockIdx.y * n * 3;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int Y = (int)(p / sw), X = (int)(p - (long long)Y * sw);
        int y0, y1, x0, x1;
        float ty, tx;
        tf_tap(Y, sy, H, y0, y1, ty);
        tf_tap(X, sx, W, x0, x1, tx);
        const float *tl = src + ((long long)y0 * W + x0) * 3, *tr = src + ((long long)y0 * W + x1) * 3;
        const float *bl = src + ((long long)y1 * W + x0) * 3, *br = src + ((long long)y1 * W + x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float m = mean.v[c];
            const float v = tf_lerp(tl[c] + m, tr[c] + m, bl[c] + m, br[c] + m, tx, ty);
            dst[p * 3 + c] = (uint8_t)((int32_t)v & 0xff); // truncation toward zero, then the low 8 bits
        }
    }
}

// q: [B][C][n] class-major; out: [B][n][C].  VEC4: C % 4 == 0 and `out` on a 16-byte boundary, so every row is.
template <bool VEC4>
__global__ __launch_bounds__(256) void seg_crf_logprob_kernel(const float *__restrict__ q, int C, long long n, float min_prob,
                                                              float *__restrict__ out) {
    const float *src = q + (long long)blockIdx.y * C * n;
    float *dst = out + (long long)blockIdx.y * n * C;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        auto prob = [&](int c) {
            const float v = src[(long long)c * n + p];
            return v < min_prob ? min_prob : v;
        };
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += prob(c);
        float *row = dst + p * C;
        if (VEC4) {
            for (int c = 0; c < C; c += 4) {
                f32x4_t r;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = logf(prob(c + k) / s);
                *reinterpret_cast<f32x4_t *>(row + c) = r;
            }
        } else {
            for (int c = 0; c < C; ++c) row[c] = logf(prob(c) / s);
        }
    }
}

// src: [B][n][C]; dst: [B][C][n]
__global__ __launch_bounds__(256) void seg_planes_from_nhwc_kernel(const float *__restrict__ src, int C, long long n, float *__restrict__ dst) {
    const float *s = src + (long long)blockIdx.y * n * C;
    float *d = dst + (long long)blockIdx.y * C * n;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        for (int c = 0; c < C; ++c) d[(long long)c * n + p] = s[p * C + c];
}

inline dim3 pixel_grid(long long n, int B) { return dim3((unsigned)std::min<long long>((n + 255) / 256, 1024), (unsigned)B); }

} // namespace

extern "C" {

int wsc_seg_preprocess_u8(wsc_ctx *ctx, const uint8_t *img_dev, int n, const int32_t *src_hw_host, const int64_t *src_off_host,
                          const float *mean_bgr_host, int H, int W, float *x_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: ctx is NULL");
    WSC_CHECK(img_dev, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: img_dev is NULL");
    WSC_CHECK(src_hw_host, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: src_hw_host is NULL");
    WSC_CHECK(src_off_host, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: src_off_host is NULL");
    WSC_CHECK(mean_bgr_host, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: mean_bgr_host is NULL");
    WSC_CHECK(x_dev, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: x_dev is NULL");
    WSC_CHECK(n >= 1 && n <= 65535, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: n=%d (1 <= n <= 65535)", n);
    WSC_CHECK(H >= 1 && W >= 1 && (long long)H * W <= INT_MAX, WSC_ERR_INVALID,
              "wsc_seg_preprocess_u8: target H=%d W=%d (both >= 1, H * W within int32)", H, W);
    std::vector<PreJob> jobs(n);
    double src_bytes = 0;
    for (int b = 0; b < n; ++b) {
        PreJob &j = jobs[b];
        j.h = src_hw_host[2 * b];
        j.w = src_hw_host[2 * b + 1];
        j.src_off = src_off_host[b];
        WSC_CHECK(j.h >= 1 && j.w >= 1 && (long long)j.h * j.w <= INT_MAX, WSC_ERR_INVALID,
                  "wsc_seg_preprocess_u8: src_hw_host[%d] = %d x %d (both >= 1, h * w within int32)", b, j.h, j.w);
        WSC_CHECK(j.src_off >= 0, WSC_ERR_INVALID, "wsc_seg_preprocess_u8: src_off_host[%d] = %lld is negative", b, (long long)j.src_off);
        src_bytes += 3.0 * j.h * j.w;
    }
    Mean3 mean = {{mean_bgr_host[0], mean_bgr_host[1], mean_bgr_host[2]}};
    WSC_HIP(hipSetDevice(ctx->device));
    WscStagedTable tab(ctx);
    const size_t jo = tab.add(jobs);
    WSC_TRY(tab.upload());
    const long long npix = (long long)H * W;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, src_bytes + 12.0 * n * (double)npix);
    hipLaunchKernelGGL(seg_preprocess_u8_kernel, pixel_grid(npix, n), dim3(256), 0, ctx->stream, img_dev, tab.at<const PreJob>(jo), mean, H,
                       W, x_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

int wsc_seg_crf_image_u8(wsc_ctx *ctx, const float *x_dev, int B, int H, int W, const float *mean_host, int sh, int sw,
                         uint8_t *out_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_seg_crf_image_u8: ctx is NULL");
    WSC_CHECK(x_dev, WSC_ERR_INVALID, "wsc_seg_crf_image_u8: x_dev is NULL");
    WSC_CHECK(mean_host, WSC_ERR_INVALID, "wsc_seg_crf_image_u8: mean_host is NULL");
    WSC_CHECK(out_dev, WSC_ERR_INVALID, "wsc_seg_crf_image_u8: out_dev is NULL");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_seg_crf_image_u8: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(H >= 1 && W >= 1 && (long long)H * W <= INT_MAX, WSC_ERR_INVALID,
              "wsc_seg_crf_image_u8: source H=%d W=%d (both >= 1, H * W within int32)", H, W);
    WSC_CHECK(sh >= 1 && sw >= 1 && (long long)sh * sw <= INT_MAX, WSC_ERR_INVALID,
              "wsc_seg_crf_image_u8: seed size sh=%d sw=%d (both >= 1, sh * sw within int32)", sh, sw);
    Mean3 mean = {{mean_host[0], mean_host[1], mean_host[2]}};
    WSC_HIP(hipSetDevice(ctx->device));
    const long long npix = (long long)sh * sw;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * (12.0 * H * W + 3.0 * (double)npix));
    hipLaunchKernelGGL(seg_crf_image_u8_kernel, pixel_grid(npix, B), dim3(256), 0, ctx->stream, x_dev, H, W, mean, sh, sw, out_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int wsc_seg_crf_logprob(wsc_ctx *ctx, const float *q_dev, int B, int C, long long n, float min_prob, float *out_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_seg_crf_logprob: ctx is NULL");
    WSC_CHECK(q_dev, WSC_ERR_INVALID, "wsc_seg_crf_logprob: q_dev is NULL");
    WSC_CHECK(out_dev, WSC_ERR_INVALID, "wsc_seg_crf_logprob: out_dev is NULL");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_seg_crf_logprob: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(C >= 1 && C <= SEG_MAX_C, WSC_ERR_INVALID, "wsc_seg_crf_logprob: C=%d (1 <= C <= %d)", C, SEG_MAX_C);
    WSC_CHECK(n >= 1 && n <= INT_MAX, WSC_ERR_INVALID, "wsc_seg_crf_logprob: n=%lld (1 <= n, within int32)", n);
    WSC_HIP(hipSetDevice(ctx->device));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 8.0 * B * C * (double)n);
    if (C % 4 == 0 && (uintptr_t)out_dev % 16 == 0)
        hipLaunchKernelGGL(seg_crf_logprob_kernel<true>, pixel_grid(n, B), dim3(256), 0, ctx->stream, q_dev, C, n, min_prob, out_dev);
    else hipLaunchKernelGGL(seg_crf_logprob_kernel<false>, pixel_grid(n, B), dim3(256), 0, ctx->stream, q_dev, C, n, min_prob, out_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int wsc_seg_planes_from_nhwc(wsc_ctx *ctx, const float *src_dev, int B, int C, long long n, float *dst_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_seg_planes_from_nhwc: ctx is NULL");
    WSC_CHECK(src_dev, WSC_ERR_INVALID, "wsc_seg_planes_from_nhwc: src_dev is NULL");
    WSC_CHECK(dst_dev, WSC_ERR_INVALID, "wsc_seg_planes_from_nhwc: dst_dev is NULL");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_seg_planes_from_nhwc: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(C >= 1 && C <= SEG_MAX_C, WSC_ERR_INVALID, "wsc_seg_planes_from_nhwc: C=%d (1 <= C <= %d)", C, SEG_MAX_C);
    WSC_CHECK(n >= 1 && n <= INT_MAX, WSC_ERR_INVALID, "wsc_seg_planes_from_nhwc: n=%lld (1 <= n, within int32)", n);
    WSC_HIP(hipSetDevice(ctx->device));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 8.0 * B * C * (double)n);
    hipLaunchKernelGGL(seg_planes_from_nhwc_kernel, pixel_grid(n, B), dim3(256), 0, ctx->stream, src_dev, C, n, dst_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

} // extern "C"
