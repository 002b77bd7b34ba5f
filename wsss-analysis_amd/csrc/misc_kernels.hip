// misc_kernels.hip -- the small HBM-bound kernels around the conv stack.
#include "common.h"

namespace {

// The door of the range guard (include/wsscam.h, WSC_ERR_RANGE) at the fp32 -> activation packs: the largest magnitude a plane
// of `fmt` holds as it is.  IEEE half: below the ceiling the saturating conversion stores (deeplab.hip's pack has the same
// test); bfloat16 and fp32: every finite value.  pack_bad is true for NaN as well (the comparison is false).
__device__ __forceinline__ float pack_limit(int fmt) { return fmt == 1 ? 65504.f : INFINITY; }
__device__ __forceinline__ bool pack_bad(float v, float lim) { return !(fabsf(v) < lim); }

// float32 NCHW [N][3][H][W] -> bf16 NHWC4 [N][H][W][4] (4th channel zero), optional lo plane.
// Replaces img.cuda() + the layout torch/cuDNN picks internally (make_cam.py:48).
// A value the planes cannot hold -- NaN, +-inf, and in the IEEE-half formats anything the saturating conversion cuts (|v| >=
// 65504) -- raises the ctx's range flag (pack_limit / pack_bad above) where the caller passes `range`.
__global__ void nchw_to_nhwc4_kernel(const float *__restrict__ x, int N, int HW, bf16_t *__restrict__ y,
                                     bf16_t *__restrict__ y_lo, int fmt, unsigned *range) {
    const long long total = (long long)N * HW;
    const float lim = pack_limit(fmt);
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / HW;
        const int p = (int)(i - n * HW);
        const float *s = x + n * 3 * HW + p;
        const float c0 = s[0], c1 = s[HW], c2 = s[2 * HW];
        bad = bad || pack_bad(c0, lim) || pack_bad(c1, lim) || pack_bad(c2, lim);
        const bf16_t h0 = f32_to_h16(c0, fmt), h1 = f32_to_h16(c1, fmt), h2 = f32_to_h16(c2, fmt);
        reinterpret_cast<uint2 *>(y)[i] = make_uint2((uint32_t)h0 | ((uint32_t)h1 << 16), (uint32_t)h2);
        if (y_lo != nullptr) {
            const bf16_t l0 = f32_to_h16(c0 - h16_to_f32(h0, fmt), fmt), l1 = f32_to_h16(c1 - h16_to_f32(h1, fmt), fmt),
                         l2 = f32_to_h16(c2 - h16_to_f32(h2, fmt), fmt);
            reinterpret_cast<uint2 *>(y_lo)[i] = make_uint2((uint32_t)l0 | ((uint32_t)l1 << 16), (uint32_t)l2);
        }
    }
    if (bad && range != nullptr) *range = 3u;
}

// The same with a zero border baked in: out [N][Hp][Wp][4], pixel (py, px) = input (py - pad, px - pad) or zeros.  The f16x3
// stem reads this buffer without bounds tests (conv_igemm.hip, CONV_FORM_STEM_ROWS): the 8-pixel window of a kernel row is 64
// contiguous, 16-byte aligned bytes of either plane.
__global__ void nchw_to_nhwc4_pad_kernel(const float *__restrict__ x, int N, int H, int W, int Hp, int Wp, int pad,
                                         bf16_t *__restrict__ y, bf16_t *__restrict__ y_lo, int fmt, unsigned *range) {
    const long long total = (long long)N * Hp * Wp;
    const long long HW = (long long)H * W;
    const float lim = pack_limit(fmt);
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int px = (int)(i % Wp);
        const long long r = i / Wp;
        const int py = (int)(r % Hp);
        const long long n = r / Hp;
        const int iy = py - pad, ix = px - pad;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            const float *s = x + n * 3 * HW + (long long)iy * W + ix;
            c0 = s[0]; c1 = s[HW]; c2 = s[2 * HW];
        }
        bad = bad || pack_bad(c0, lim) || pack_bad(c1, lim) || pack_bad(c2, lim);
        const bf16_t h0 = f32_to_h16(c0, fmt), h1 = f32_to_h16(c1, fmt), h2 = f32_to_h16(c2, fmt);
        reinterpret_cast<uint2 *>(y)[i] = make_uint2((uint32_t)h0 | ((uint32_t)h1 << 16), (uint32_t)h2);
        if (y_lo != nullptr) {
            const bf16_t l0 = f32_to_h16(c0 - h16_to_f32(h0, fmt), fmt), l1 = f32_to_h16(c1 - h16_to_f32(h1, fmt), fmt),
                         l2 = f32_to_h16(c2 - h16_to_f32(h2, fmt), fmt);
            reinterpret_cast<uint2 *>(y_lo)[i] = make_uint2((uint32_t)l0 | ((uint32_t)l1 << 16), (uint32_t)l2);
        }
    }
    if (bad && range != nullptr) *range = 3u;
}

// Strided pixel gather into a channel range of a wider tensor: y[(n, ho, wo)][0 .. C) = x[n][ho * stride][wo * stride][0 .. C),
// rows of y `ldy` elements apart -- the shortcut input of a ResNet stage's first block, placed beside conv2's output so that
// conv3 and the 1x1 projection are ONE GEMM over the concatenated channels (net.hip build_resnet50_backbone).  16 bytes per thread.
__global__ __launch_bounds__(256) void gather_strided_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, int H, int W,
                                                             int C8, int stride, int Ho, int Wo, bf16_t *__restrict__ y,
                                                             bf16_t *__restrict__ y_lo, int ldy, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        long long m = i / C8;
        const int wo = (int)(m % Wo);
        const long long r = m / Wo;
        const int ho = (int)(r % Ho);
        const long long n = r / Ho;
        const long long src = (((n * H + (long long)ho * stride) * W + (long long)wo * stride) * C8 + c8) * 8;
        const long long dst = m * ldy + c8 * 8;
        *reinterpret_cast<uint4 *>(y + dst) = *reinterpret_cast<const uint4 *>(x + src);
        if (x_lo != nullptr) *reinterpret_cast<uint4 *>(y_lo + dst) = *reinterpret_cast<const uint4 *>(x_lo + src);
    }
}

// x = relu(head); cam = x[0] + x[1].flip(-1)   (resnet50_cam.py:66-68, vgg16_cam.py:49-50)
// head: fp32 [2B][h][w][Cs] (NHWC, first C channels valid) -> cam fp32 [B][C][h][w]
__global__ void flip_add_kernel(const float *__restrict__ head, int B, int h, int w, int C, int Cs,
                                float *__restrict__ cam) {
    const long long total = (long long)B * C * h * w;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % w);
        long long r = i / w;
        const int yy = (int)(r % h);
        r /= h;
        const int c = (int)(r % C);
        const int b = (int)(r / C);
        const float a = head[(((long long)(2 * b) * h + yy) * w + xx) * Cs + c];
        const float f = head[(((long long)(2 * b + 1) * h + yy) * w + (w - 1 - xx)) * Cs + c];
        cam[i] = relu_keep_nan(a) + relu_keep_nan(f);
    }
}

// Classifier branch of vgg16_cam.py:34-36 on sample 0 of each image:
// score[b][c] = sigmoid(bias[c] + sum_f Wc[c][f] * mean_hw feat[sample_stride*b][.][f])
// Global pooling + Linear + Sigmoid of the classifier branch, in two kernels: (1) a block per (image, 64 channels), lane =
// channel, the positions dealt to the block's GAP_WAVES waves in contiguous runs: every wave sums its run in order (fp32, eight
// independent loads in flight) and wave 0 adds the GAP_WAVES partial sums in run order -- a fixed summation order, whatever
// the batch.  (One wave per (image, 64 channels) walked all 1600 positions of a 40 x 40 map alone: 200 dependent round
// trips, 450 us for 16 images; one block per image before that: 1.9 ms.)  (2) one block per image for the C dot products.
// feat NHWC half / bf16 (+ lo plane).  hw < 0 selects the global max of m7 (m7_cam.py:32-35: MaxPool 2x2 then
// AdaptiveMaxPool2d((1,1))).
constexpr int GAP_WAVES = 16;
__global__ __launch_bounds__(64 * GAP_WAVES) void gap_kernel(const bf16_t *__restrict__ feat, const bf16_t *__restrict__ feat_lo,
                                                             int hw, int F, float *__restrict__ gap, int fmt, int sample_stride) {
    __shared__ float part[GAP_WAVES][64];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    const bool use_max = hw < 0; // m7: AdaptiveMaxPool2d((1,1)) instead of the average
    const int npix = use_max ? -hw : hw;
    const int run = (npix + GAP_WAVES - 1) / GAP_WAVES;
    const int pb = wv * run, pe = min(npix, pb + run);
    float s = use_max ? -3.0e38f : 0.f;
    if (f < F) {
        const long long img = (long long)(sample_stride * b) * npix * F;
        const bf16_t *f0 = feat + img + f;
        const bf16_t *l0 = feat_lo ? feat_lo + img + f : nullptr;
        int p = pb;
        for (; p + 8 <= pe; p += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = h16_to_f32(f0[(long long)(p + u) * F], fmt);
                if (l0) v[u] += h16_to_f32(l0[(long long)(p + u) * F], fmt);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s = use_max ? max_keep_nan(s, v[u]) : s + v[u];
        }
        for (; p < pe; ++p) {
            float v = h16_to_f32(f0[(long long)p * F], fmt);
            if (l0) v += h16_to_f32(l0[(long long)p * F], fmt);
            s = use_max ? max_keep_nan(s, v) : s + v;
        }
    }
    part[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && f < F) {
        float t = part[0][lane];
        for (int k = 1; k < GAP_WAVES; ++k) t = use_max ? max_keep_nan(t, part[k][lane]) : t + part[k][lane];
        gap[(long long)b * F + f] = use_max ? t : t / (float)npix;
    }
}

__global__ void linear_sigmoid_kernel(const float *__restrict__ gapbuf, int F, const float *__restrict__ Wc,
                                      const float *__restrict__ bias, int C, float *__restrict__ score) {
    extern __shared__ float gap[]; // F floats
    const int b = blockIdx.x;
    for (int f = threadIdx.x; f < F; f += blockDim.x) gap[f] = gapbuf[(long long)b * F + f];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int c = wv; c < C; c += nw) {
        float s = 0.f;
        for (int f = lane; f < F; f += 64) s += gap[f] * Wc[(long long)c * F + f];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) score[(long long)b * C + c] = 1.f / (1.f + expf(-(s + (bias ? bias[c] : 0.f))));
    }
}

__global__ void bf16_to_f32_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, size_t n,
                                   float *__restrict__ y, int fmt) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = h16_to_f32(x[i], fmt);
        if (x_lo) v += h16_to_f32(x_lo[i], fmt);
        y[i] = v;
    }
}

// generic layout changes for the single-layer entry point (wsc_conv2d_nchw)
__global__ void nchw_to_nhwc_kernel(const float *__restrict__ x, int N, int C, int HW, bf16_t *__restrict__ y,
                                    bf16_t *__restrict__ y_lo, int fmt, unsigned *range) {
    const long long total = (long long)N * C * HW;
    const float lim = pack_limit(fmt);
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long r = i / C;
        const int p = (int)(r % HW);
        const long long n = r / HW;
        const float v = x[(n * C + c) * HW + p];
        bad = bad || pack_bad(v, lim);
        const bf16_t h = f32_to_h16(v, fmt);
        y[i] = h;
        if (y_lo) y_lo[i] = f32_to_h16(v - h16_to_f32(h, fmt), fmt);
    }
    if (bad && range != nullptr) *range = (unsigned)C;
}
__global__ void nhwc_to_nchw_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, int N, int C,
                                    int HW, float *__restrict__ y, int fmt) {
    const long long total = (long long)N * C * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const long long r = i / HW;
        const int c = (int)(r % C);
        const long long n = r / C;
        const long long src = (n * HW + p) * C + c;
        float v = h16_to_f32(x[src], fmt);
        if (x_lo) v += h16_to_f32(x_lo[src], fmt);
        y[i] = v;
    }
}

// ---- WSC_PREC_F32: the same maps on one plane of fp32 (the launch functions take them for an Act of that precision).
// HBM-bound, 16 bytes per access where the layout has them.
__global__ void nchw_to_nhwc4_f32_kernel(const float *__restrict__ x, int N, int HW, f32x4_t *__restrict__ y, unsigned *range) {
    const long long total = (long long)N * HW;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / HW;
        const int p = (int)(i - n * HW);
        const float *s = x + n * 3 * HW + p;
        const float c0 = s[0], c1 = s[HW], c2 = s[2 * HW];
        bad = bad || pack_bad(c0, INFINITY) || pack_bad(c1, INFINITY) || pack_bad(c2, INFINITY);
        y[i] = f32x4_t{c0, c1, c2, 0.f};
    }
    if (bad && range != nullptr) *range = 3u;
}
// gap_kernel's decomposition and summation order on fp32 features
__global__ __launch_bounds__(64 * GAP_WAVES) void gap_f32_kernel(const float *__restrict__ feat, int hw, int F, float *__restrict__ gap,
                                                                 int sample_stride) {
    __shared__ float part[GAP_WAVES][64];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    const bool use_max = hw < 0;
    const int npix = use_max ? -hw : hw;
    const int run = (npix + GAP_WAVES - 1) / GAP_WAVES;
    const int pb = wv * run, pe = min(npix, pb + run);
    float s = use_max ? -3.0e38f : 0.f;
    if (f < F) {
        const float *f0 = feat + (long long)(sample_stride * b) * npix * F + f;
        int p = pb;
        for (; p + 8 <= pe; p += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = f0[(long long)(p + u) * F];
#pragma unroll
            for (int u = 0; u < 8; ++u) s = use_max ? max_keep_nan(s, v[u]) : s + v[u];
        }
        for (; p < pe; ++p) s = use_max ? max_keep_nan(s, f0[(long long)p * F]) : s + f0[(long long)p * F];
    }
    part[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && f < F) {
        float t = part[0][lane];
        for (int k = 1; k < GAP_WAVES; ++k) t = use_max ? max_keep_nan(t, part[k][lane]) : t + part[k][lane];
        gap[(long long)b * F + f] = use_max ? t : t / (float)npix;
    }
}
// layout changes of the single-layer entry point; TO_NHWC: y[n][p][c] = x[n][c][p], else y[n][c][p] = x[n][p][c]
template <bool TO_NHWC>
__global__ void relayout_f32_kernel(const float *__restrict__ x, int N, int C, int HW, float *__restrict__ y, unsigned *range) {
    const long long total = (long long)N * C * HW;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int inner = TO_NHWC ? C : HW, outer = TO_NHWC ? HW : C;
        const int a = (int)(i % inner);
        const long long r = i / inner;
        const int b = (int)(r % outer);
        const long long n = r / outer;
        const float v = x[(n * inner + a) * outer + b];
        bad = bad || pack_bad(v, INFINITY);
        y[i] = v;
    }
    if (bad && range != nullptr) *range = (unsigned)C;
}

} // namespace

int launch_nchw_to_nhwc4(wsc_ctx *ctx, const float *x, int N, int H, int W, Act y, unsigned *range) {
    const long long total = (long long)N * H * W;
    const bool f32 = y.is_f32();
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)total * (12 + (f32 ? 16 : 8)));
    if (f32)
        hipLaunchKernelGGL(nchw_to_nhwc4_f32_kernel, dim3(wsc_grid_for(total)), dim3(256), 0, ctx->stream, x, N, H * W, (f32x4_t *)y.f32(), range);
    else
        hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(wsc_grid_for(total)), dim3(256), 0, ctx->stream, x, N, H * W, y.h16(), y.h16_lo(),
                           y.fmt(), range);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_nchw_to_nhwc4_pad(wsc_ctx *ctx, const float *x, int N, int H, int W, int Hp, int Wp, int pad, Act y, unsigned *range) {
    WSC_CHECK(!y.is_f32(), WSC_ERR_INVALID, "the padded NHWC4 input is a half-mode path");
    const long long total = (long long)N * Hp * Wp;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)N * H * W * 12 + (double)total * (y.lo ? 16 : 8));
    hipLaunchKernelGGL(nchw_to_nhwc4_pad_kernel, dim3(wsc_grid_for(total)), dim3(256), 0, ctx->stream, x, N, H, W, Hp, Wp, pad, y.h16(),
                       y.h16_lo(), y.fmt(), range);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_gather_strided(wsc_ctx *ctx, Act x, int N, int H, int W, int C, int stride, int Ho, int Wo, Act y, int ldy) {
    WSC_CHECK(!x.is_f32() && y.prec == x.prec, WSC_ERR_INVALID, "gather: 16-bit planes of one precision only");
    WSC_CHECK(C % 8 == 0 && ldy % 8 == 0, WSC_ERR_INVALID, "gather: C=%d, pitch=%d not multiples of 8", C, ldy);
    const long long total = (long long)N * Ho * Wo * (C / 8);
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)total * 32 * (x.lo ? 2 : 1));
    hipLaunchKernelGGL(gather_strided_kernel, dim3(wsc_grid_for(total)), dim3(256), 0, ctx->stream, x.h16(), x.h16_lo(), H, W, C / 8, stride,
                       Ho, Wo, y.h16(), y.h16_lo(), ldy, total);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_flip_add(wsc_ctx *ctx, const float *head, int B, int h, int w, int C, int Cs, float *cam) {
    const long long total = (long long)B * C * h * w;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)total * 12);
    hipLaunchKernelGGL(flip_add_kernel, dim3(wsc_grid_for(total)), dim3(256), 0, ctx->stream, head, B, h, w, C, Cs,
                       cam);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_gap_linear_sigmoid(wsc_ctx *ctx, Act feat, int B, int hw, int F, const float *Wc, const float *bias, int C, float *score,
                              int sample_stride) {
    float *gapbuf = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, sizeof(float) * (size_t)B * F, (void **)&gapbuf));
    WscCachedGuard gapbuf_guard(ctx, gapbuf);
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)B), block(64 * GAP_WAVES);
    if (feat.is_f32())
        hipLaunchKernelGGL(gap_f32_kernel, grid, block, 0, ctx->stream, (const float *)feat.f32(), hw, F, gapbuf, sample_stride);
    else
        hipLaunchKernelGGL(gap_kernel, grid, block, 0, ctx->stream, (const bf16_t *)feat.h16(), (const bf16_t *)feat.h16_lo(), hw, F,
                           gapbuf, feat.fmt(), sample_stride);
    hipLaunchKernelGGL(linear_sigmoid_kernel, dim3(B), dim3(256), F * sizeof(float), ctx->stream, (const float *)gapbuf, F, Wc, bias, C,
                       score);
    WSC_HIP(hipGetLastError());
    gapbuf_guard.free_now(); // stream-ordered reuse
    return WSC_OK;
}

int launch_act_to_f32(wsc_ctx *ctx, Act x, size_t n, float *y) {
    if (x.is_f32()) { // (the activation is the fp32 tensor already)
        WSC_HIP(hipMemcpyAsync(y, x.f32(), n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return WSC_OK;
    }
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(wsc_grid_for((long long)n)), dim3(256), 0, ctx->stream, (const bf16_t *)x.h16(),
                       (const bf16_t *)x.h16_lo(), n, y, x.fmt());
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_nchw_to_nhwc(wsc_ctx *ctx, const float *x, int N, int C, int HW, Act y, unsigned *range) {
    const dim3 grid(wsc_grid_for((long long)N * C * HW));
    if (y.is_f32())
        hipLaunchKernelGGL(relayout_f32_kernel<true>, grid, dim3(256), 0, ctx->stream, x, N, C, HW, y.f32(), range);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid, dim3(256), 0, ctx->stream, x, N, C, HW, y.h16(), y.h16_lo(), y.fmt(), range);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_nhwc_to_nchw(wsc_ctx *ctx, Act x, int N, int C, int HW, float *y) {
    const dim3 grid(wsc_grid_for((long long)N * C * HW));
    if (x.is_f32())
        hipLaunchKernelGGL(relayout_f32_kernel<false>, grid, dim3(256), 0, ctx->stream, (const float *)x.f32(), N, C, HW, y, (unsigned *)nullptr);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid, dim3(256), 0, ctx->stream, (const bf16_t *)x.h16(), (const bf16_t *)x.h16_lo(), N,
                           C, HW, y, x.fmt());
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}
