// pool.hip -- every K x K pooling window of the library on an NHWC activation: one geometry (common.h PoolGeom: PoolRule says how
// the output size and the padding before follow from the input size), one launcher, one kernel family.
//   nn.MaxPool2d(k, stride, pad)   the torch-side nets: resnet50.py:64 (3 x 3 / 2 / 1), common_cnn.py:131-132 (2 x 2 / 2)
//   TF `SAME` 3 x 3                max_pool at stride 2 / 1 and avg_pool at stride 1 of the SEC / DSRG DeepLab nets' build_block
//                                  (DSRG.py:229-246, SEC.py:173-188)
//   TF / Keras MaxPooling2D        window 2 or 3, stride 1 or 2, `SAME` or `VALID`: the pools a Keras-side session's architecture
//                                  file gives the CAM nets (02_cues/demo.py:104-124 model_from_json; the `pool_spec` of net.hip)
// A window walks the image, taps outside it are skipped: padding never wins a maximum (-inf, not 0 -- the pools see signed
// values), the average divides by the number of IN-IMAGE taps (4 at a corner, 6 on an edge).  A value of the 16-bit planes is
// hi + lo, exact in fp32 (11 + 11 or 8 + 8 significant bits).  Max: the maximum of those values, split again -- value-exact, it
// is one of the inputs.  Average: summed and divided in double (9 fp32 terms: exact but for the final rounding), then split.
// HBM-bound maps with no reuse beyond the window's footprint: one thread per output vector, no LDS.  (No float a * b + c in
// this file: it needs no contraction flag.)
// Kernels, by the data alone (launch_pool):
//   fp32 plane                              pool_f32_kernel<K, AVG>, 4 channels per thread
//   IEEE half, max, N * Ho <= 65535         maxpool_f16_kernel (one plane) / maxpool_f16x2_kernel (two): a block row per output row
//   everything else                         pool_h16_kernel<K, AVG>, 8 channels per thread
// K = 2, 3: the taps unrolled; K = 0: the window is PoolArgs::k (the layer entry's other windows).  AVG exists for K = 3.
#include "common.h"

#include <cmath>

namespace {

struct PoolArgs {
    int N, H, W, C, Ho, Wo;
    int k, stride, pad_t, pad_l;
};

// 8 channels at element `o` of the 16-bit plane(s) as their fp32 values hi (+ lo).  two: the lo plane is there -- an argument, so
// that a kernel of two-plane activations says `true` and carries no test (the compiler does not drop one on the pointer)
__device__ __forceinline__ void load8(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, bool two, long long o, int fmt,
                                      float f[8]) {
    const uint4 v = *reinterpret_cast<const uint4 *>(x + o);
    const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = h16_to_f32((bf16_t)(vw[j] & 0xffffu), fmt);
        f[2 * j + 1] = h16_to_f32((bf16_t)(vw[j] >> 16), fmt);
    }
    if (two) {
        const uint4 l = *reinterpret_cast<const uint4 *>(x_lo + o);
        const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[2 * j] += h16_to_f32((bf16_t)(lw[j] & 0xffffu), fmt);
            f[2 * j + 1] += h16_to_f32((bf16_t)(lw[j] >> 16), fmt);
        }
    }
}
// ... and 8 fp32 values split into the plane(s) at element `o`: hi = the value rounded, lo = what is left of it
__device__ __forceinline__ void store8(const float r[8], bf16_t *__restrict__ y, bf16_t *__restrict__ y_lo, bool two, long long o, int fmt) {
    uint32_t hw[4], lw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bf16_t h0 = f32_to_h16(r[2 * j], fmt), h1 = f32_to_h16(r[2 * j + 1], fmt);
        hw[j] = (uint32_t)h0 | ((uint32_t)h1 << 16);
        const bf16_t l0 = f32_to_h16(r[2 * j] - h16_to_f32(h0, fmt), fmt);
        const bf16_t l1 = f32_to_h16(r[2 * j + 1] - h16_to_f32(h1, fmt), fmt);
        lw[j] = (uint32_t)l0 | ((uint32_t)l1 << 16);
    }
    *reinterpret_cast<uint4 *>(y + o) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
    if (two) *reinterpret_cast<uint4 *>(y_lo + o) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
}

// 16-bit planes of either format, the lo plane optional, 8 channels per thread
template <int K, bool AVG>
__global__ __launch_bounds__(256) void pool_h16_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, PoolArgs a,
                                                       bf16_t *__restrict__ y, bf16_t *__restrict__ y_lo, int fmt) {
    const int k = K ? K : a.k;
    constexpr int UNROLL = K ? K : 1; // (a run-time window: the loops stay loops)
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
#pragma unroll UNROLL
        for (int dy = 0; dy < k; ++dy) {
            const int hi = ho * a.stride - a.pad_t + dy;
            if ((unsigned)hi >= (unsigned)a.H) continue;
#pragma unroll UNROLL
            for (int dx = 0; dx < k; ++dx) {
                const int wi = wo * a.stride - a.pad_l + dx;
                if ((unsigned)wi >= (unsigned)a.W) continue;
                float f[8];
                load8(x, x_lo, x_lo != nullptr, (((long long)n * a.H + hi) * a.W + wi) * a.C + c8 * 8, fmt, f);
                ++cnt;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (AVG) sum[j] += (double)f[j];
                    else best[j] = max_keep_nan(best[j], f[j]);
                }
            }
        }
        if (AVG) {
#pragma unroll
            for (int j = 0; j < 8; ++j) best[j] = (float)(sum[j] / (double)cnt);
        }
        store8(best, y, y_lo, y_lo != nullptr, (((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c8 * 8, fmt);
    }
}

// WSC_PREC_F32: one plane of fp32, 4 channels per thread; max is bit-exact, the average is the double sum rounded once
template <int K, bool AVG>
__global__ __launch_bounds__(256) void pool_f32_kernel(const float *__restrict__ x, PoolArgs a, float *__restrict__ y) {
    const int k = K ? K : a.k;
    constexpr int UNROLL = K ? K : 1; // (a run-time window: the loops stay loops)
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
#pragma unroll UNROLL
        for (int dy = 0; dy < k; ++dy) {
            const int hi = ho * a.stride - a.pad_t + dy;
            if ((unsigned)hi >= (unsigned)a.H) continue;
#pragma unroll UNROLL
            for (int dx = 0; dx < k; ++dx) {
                const int wi = wo * a.stride - a.pad_l + dx;
                if ((unsigned)wi >= (unsigned)a.W) continue;
                const f32x4_t v = *reinterpret_cast<const f32x4_t *>(x + ((((long long)n * a.H + hi) * a.W + wi) * a.C + c4 * 4));
                ++cnt;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (AVG) sum[j] += (double)v[j];
                    else best[j] = max_keep_nan(best[j], v[j]);
                }
            }
        }
        if (AVG) {
#pragma unroll
            for (int j = 0; j < 4; ++j) best[j] = (float)(sum[j] / (double)cnt);
        }
        *reinterpret_cast<f32x4_t *>(y + ((((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c4 * 4)) = best;
    }
}

// The maximum for IEEE-half activations with one precision plane (the default path): taken on the halves themselves
// (v_pk_max_f16, two channels per instruction -- exact, no conversion), one block row per output row (blockIdx.y = n * Ho + ho:
// no 64-bit index divisions).  8 channels = one 16-byte load per tap.
__global__ __launch_bounds__(256) void maxpool_f16_kernel(const bf16_t *__restrict__ x, int H, int W, int C, int k, int stride,
                                                          int pad_t, int pad_l, int Ho, int Wo, bf16_t *__restrict__ y) {
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
    const int C8 = C >> 3;
    const int row = blockIdx.y; // n * Ho + ho
    const int n = row / Ho, ho = row - n * Ho;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Wo * C8; i += gridDim.x * blockDim.x) {
        const int wo = i / C8, c8 = i - wo * C8;
        const h2_t lowest = {(_Float16)-65504.f, (_Float16)-65504.f};
        h2_t best[4] = {lowest, lowest, lowest, lowest};
        for (int dy = 0; dy < k; ++dy) {
            const int hi = ho * stride - pad_t + dy;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int dx = 0; dx < k; ++dx) {
                const int wi = wo * stride - pad_l + dx;
                if ((unsigned)wi >= (unsigned)W) continue;
                const uint4 v = *reinterpret_cast<const uint4 *>(x + ((((long long)n * H + hi) * W + wi) * C + c8 * 8));
                const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) best[j] = __builtin_elementwise_max(best[j], __builtin_bit_cast(h2_t, vw[j]));
            }
        }
        *reinterpret_cast<uint4 *>(y + (((long long)row * Wo + wo) * C + c8 * 8)) =
            make_uint4(__builtin_bit_cast(uint32_t, best[0]), __builtin_bit_cast(uint32_t, best[1]),
                       __builtin_bit_cast(uint32_t, best[2]), __builtin_bit_cast(uint32_t, best[3]));
    }
}

// The same mapping for the two-plane half activations of the f16x3 mode, on the values hi + lo.  pool_h16_kernel spends a 64-bit
// index division chain per 8 channels and ran the ResNet stem's pool at 3.75 TB/s (142 us for 532 MB).
__global__ __launch_bounds__(256) void maxpool_f16x2_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ x_lo, int H, int W,
                                                            int C, int k, int stride, int pad_t, int pad_l, int Ho, int Wo,
                                                            bf16_t *__restrict__ y, bf16_t *__restrict__ y_lo) {
    const int C8 = C >> 3;
    const int row = blockIdx.y; // n * Ho + ho
    const int n = row / Ho, ho = row - n * Ho;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Wo * C8; i += gridDim.x * blockDim.x) {
        const int wo = i / C8, c8 = i - wo * C8;
        float best[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = -3.0e38f;
        for (int dy = 0; dy < k; ++dy) {
            const int hi = ho * stride - pad_t + dy;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int dx = 0; dx < k; ++dx) {
                const int wi = wo * stride - pad_l + dx;
                if ((unsigned)wi >= (unsigned)W) continue;
                float f[8];
                load8(x, x_lo, true, (((long long)n * H + hi) * W + wi) * C + c8 * 8, 1, f);
#pragma unroll
                for (int j = 0; j < 8; ++j) best[j] = fmaxf(best[j], f[j]);
            }
        }
        store8(best, y, y_lo, true, ((long long)row * Wo + wo) * C + c8 * 8, 1);
    }
}

template <int K, bool AVG>
void launch_generic(wsc_ctx *ctx, Act x, const PoolArgs &a, Act y) {
    const long long total = (long long)a.N * a.Ho * a.Wo * (a.C / (x.is_f32() ? 4 : 8));
    const dim3 grid(wsc_grid_for(total)), block(256);
    if (x.is_f32()) hipLaunchKernelGGL((pool_f32_kernel<K, AVG>), grid, block, 0, ctx->stream, x.f32(), a, y.f32());
    else
        hipLaunchKernelGGL((pool_h16_kernel<K, AVG>), grid, block, 0, ctx->stream, x.h16(), x.h16_lo(), a, y.h16(), y.h16_lo(), x.fmt());
}

} // namespace

int launch_pool(wsc_ctx *ctx, Act x, int N, int H, int W, int C, const PoolGeom &g, Act y) {
    WSC_CHECK(x && y && y.prec == x.prec, WSC_ERR_INVALID, "pool: input and output of different precisions");
    WSC_CHECK(C > 0 && C % 8 == 0, WSC_ERR_INVALID, "pool: C=%d not a multiple of 8", C);
    // (2 pad_before <= k: every window has a tap inside the image, so no output is the identity of the maximum or 0 / 0)
    WSC_CHECK(N > 0 && H > 0 && W > 0 && g.Ho >= 1 && g.Wo >= 1 && g.k >= 1 && g.stride >= 1 && g.pad_t >= 0 && g.pad_l >= 0 &&
                  2 * g.pad_t <= g.k && 2 * g.pad_l <= g.k,
              WSC_ERR_INVALID, "pool: window %d stride %d padding %d / %d before on %d x %d x %d -> %d x %d", g.k, g.stride, g.pad_t, g.pad_l,
              N, H, W, g.Ho, g.Wo);
    WSC_CHECK(!g.avg || (g.k == 3 && g.stride == 1), WSC_ERR_INVALID, "pool: the average is 3 x 3 at stride 1, got window %d stride %d", g.k,
              g.stride);
    const PoolArgs a = {N, H, W, C, g.Ho, g.Wo, g.k, g.stride, g.pad_t, g.pad_l};
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, ((double)N * H * W * C + (double)N * g.Ho * g.Wo * C) * (x.is_f32() || x.lo ? 4 : 2));
    const bool rows = x.fmt() == 1 && !g.avg && (long long)N * g.Ho <= 65535; // IEEE half, one block row per output row
    const dim3 row_grid((unsigned)((g.Wo * (C / 8) + 255) / 256), (unsigned)(N * g.Ho));
    if (rows && !x.lo && !y.lo)
        hipLaunchKernelGGL(maxpool_f16_kernel, row_grid, dim3(256), 0, ctx->stream, x.h16(), H, W, C, g.k, g.stride, g.pad_t, g.pad_l, g.Ho,
                           g.Wo, y.h16());
    else if (rows && x.lo && y.lo)
        hipLaunchKernelGGL(maxpool_f16x2_kernel, row_grid, dim3(256), 0, ctx->stream, x.h16(), x.h16_lo(), H, W, C, g.k, g.stride, g.pad_t,
                           g.pad_l, g.Ho, g.Wo, y.h16(), y.h16_lo());
    else if (g.avg) launch_generic<3, true>(ctx, x, a, y);
    else if (g.k == 2) launch_generic<2, false>(ctx, x, a, y);
    else if (g.k == 3) launch_generic<3, false>(ctx, x, a, y);
    else launch_generic<0, false>(ctx, x, a, y);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

// ---- the gradient with respect to the input (the backward pass of the SEC / DSRG nets, fp32 planes only) -----------------------
namespace {

// Gather form: one thread per 4 channels of an INPUT pixel walks the windows that cover it (<= 4 at stride 2, <= 9 at stride 1)
// in row-major order of (ho, wo).  Max: the window's first maximum in row-major window order is recomputed from x (strict >, the
// rule of torch's and TensorFlow's kernels; padding is never a candidate) and dy goes to that tap alone.  Average: dy / (in-image
// tap count) to every tap.  No atomics, no argmax plane; the sum is in window order.
template <bool AVG>
__global__ __launch_bounds__(256) void pool_grad_f32_kernel(const float *__restrict__ x, const float *__restrict__ dy, PoolArgs a,
                                                            float *__restrict__ dx) {
    const int C4 = a.C >> 2;
    const long long total = (long long)a.N * a.H * a.W * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long long pix = i / C4;
        const int wi = (int)(pix % a.W);
        pix /= a.W;
        const int hi = (int)(pix % a.H);
        const int n = (int)(pix / a.H);
        // windows ho with ho stride - pad_t <= hi <= ho stride - pad_t + k - 1
        const int nh = hi + a.pad_t - a.k + 1, nw = wi + a.pad_l - a.k + 1;
        const int ho_lo = nh > 0 ? (nh + a.stride - 1) / a.stride : 0, wo_lo = nw > 0 ? (nw + a.stride - 1) / a.stride : 0;
        const int ho_hi = min((hi + a.pad_t) / a.stride, a.Ho - 1), wo_hi = min((wi + a.pad_l) / a.stride, a.Wo - 1);
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        for (int ho = ho_lo; ho <= ho_hi; ++ho)
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                const int h0 = ho * a.stride - a.pad_t, w0 = wo * a.stride - a.pad_l;
                const f32x4_t g = *reinterpret_cast<const f32x4_t *>(dy + ((((long long)n * a.Ho + ho) * a.Wo + wo) * a.C + c4 * 4));
                if (AVG) {
                    const int cnt = (min(h0 + a.k, a.H) - max(h0, 0)) * (min(w0 + a.k, a.W) - max(w0, 0));
                    const float fc = (float)cnt;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += g[j] / fc;
                } else {
                    f32x4_t best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    int arg[4] = {-1, -1, -1, -1};
                    for (int dy_ = 0; dy_ < a.k; ++dy_) {
                        const int h = h0 + dy_;
                        if ((unsigned)h >= (unsigned)a.H) continue;
                        for (int dx_ = 0; dx_ < a.k; ++dx_) {
                            const int w = w0 + dx_;
                            if ((unsigned)w >= (unsigned)a.W) continue;
                            const f32x4_t v = *reinterpret_cast<const f32x4_t *>(x + ((((long long)n * a.H + h) * a.W + w) * a.C + c4 * 4));
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (v[j] > best[j]) {
                                    best[j] = v[j];
                                    arg[j] = dy_ * a.k + dx_;
                                }
                        }
                    }
                    const int mine = (hi - h0) * a.k + (wi - w0);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (arg[j] == mine) acc[j] += g[j];
                }
            }
        *reinterpret_cast<f32x4_t *>(dx + ((((long long)n * a.H + hi) * a.W + wi) * a.C + c4 * 4)) = acc;
    }
}

} // namespace

int launch_pool_grad(wsc_ctx *ctx, const float *x, const float *dy, int N, int H, int W, int C, const PoolGeom &g, float *dx) {
    WSC_CHECK(x && dy && dx, WSC_ERR_INVALID, "pool gradient: null argument");
    WSC_CHECK(C > 0 && C % 4 == 0, WSC_ERR_INVALID, "pool gradient: C=%d not a multiple of 4", C);
    WSC_CHECK(N > 0 && H > 0 && W > 0 && g.Ho >= 1 && g.Wo >= 1 && g.k >= 1 && g.stride >= 1 && g.pad_t >= 0 && g.pad_l >= 0 &&
                  2 * g.pad_t <= g.k && 2 * g.pad_l <= g.k,
              WSC_ERR_INVALID, "pool gradient: window %d stride %d padding %d / %d before on %d x %d x %d -> %d x %d", g.k, g.stride, g.pad_t,
              g.pad_l, N, H, W, g.Ho, g.Wo);
    const PoolArgs a = {N, H, W, C, g.Ho, g.Wo, g.k, g.stride, g.pad_t, g.pad_l};
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (2.0 * N * H * W * C + (double)N * g.Ho * g.Wo * C) * 4);
    const dim3 grid(wsc_grid_for((long long)N * H * W * (C / 4))), block(256);
    if (g.avg) hipLaunchKernelGGL((pool_grad_f32_kernel<true>), grid, block, 0, ctx->stream, x, dy, a, dx);
    else hipLaunchKernelGGL((pool_grad_f32_kernel<false>), grid, block, 0, ctx->stream, x, dy, a, dx);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

// ---- the per-layer entries: float32 NHWC through the activation planes of a precision, the production launcher unchanged ------
namespace {

int check_tensor(const char *who, wsc_ctx *ctx, const float *x_dev, const float *y_dev, int N, int H, int W, int C, int precision) {
    WSC_CHECK(ctx && x_dev && y_dev, WSC_ERR_INVALID, "%s: null argument", who);
    WSC_CHECK(precision >= WSC_PREC_BF16 && precision <= WSC_PREC_F32, WSC_ERR_INVALID, "unknown precision %d", precision);
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, WSC_ERR_INVALID, "%s: %d x %d x %d x %d (C a multiple of 8)", who, N, H, W, C);
    return WSC_OK;
}

// stage -> launch_pool -> unstage (the layout change of the single-layer entry with one "pixel" per sample row: NHWC stays
// NHWC, the values take the planes)
int pool_staged(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, const PoolGeom &g, int precision, float *y_dev) {
    WSC_HIP(hipSetDevice(ctx->device));
    const wsc_precision prec = (wsc_precision)precision;
    const size_t in_e = (size_t)N * H * W * C, out_e = (size_t)N * g.Ho * g.Wo * C;
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, act_bytes(in_e, prec) + act_bytes(out_e, prec), &ws));
    char *p = (char *)ws;
    const Act xi = act_carve(p, in_e, prec), yo = act_carve(p, out_e, prec);
    WSC_TRY(launch_nchw_to_nhwc(ctx, x_dev, (int)((size_t)N * H * W), C, 1, xi, layer_door(ctx, xi.prec)));
    WSC_TRY(launch_pool(ctx, xi, N, H, W, C, g, yo));
    return launch_act_to_f32(ctx, yo, out_e, y_dev);
}

} // namespace

extern "C" {

int wsc_maxpool_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int k, int stride, int pad, int precision,
                     float *y_dev) {
    WSC_TRY(check_tensor("wsc_maxpool_nhwc", ctx, x_dev, y_dev, N, H, W, C, precision));
    WSC_CHECK(k >= 1 && stride >= 1 && pad >= 0 && 2 * pad <= k, WSC_ERR_INVALID,
              "wsc_maxpool_nhwc: window %d stride %d padding %d (padding at most half the window)", k, stride, pad);
    PoolGeom g;
    WSC_CHECK(H + 2 * pad >= k && W + 2 * pad >= k && pool_geom(POOL_TORCH, k, stride, pad, false, H, W, &g), WSC_ERR_INVALID,
              "wsc_maxpool_nhwc: a %d x %d map is smaller than the window %d", H, W, k);
    return pool_staged(ctx, x_dev, N, H, W, C, g, precision, y_dev);
}

int wsc_pool_same_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int avg, int stride, int precision, float *y_dev) {
    WSC_TRY(check_tensor("wsc_pool_same_nhwc", ctx, x_dev, y_dev, N, H, W, C, precision));
    PoolGeom g;
    WSC_CHECK((stride == 1 || stride == 2) && (!avg || stride == 1) && pool_geom(POOL_TF_SAME, 3, stride, 0, avg != 0, H, W, &g),
              WSC_ERR_INVALID, "wsc_pool_same_nhwc: 3x3 max at stride 1 / 2 or 3x3 average at stride 1, got stride %d", stride);
    return pool_staged(ctx, x_dev, N, H, W, C, g, precision, y_dev);
}

int wsc_pool_tf_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int k, int stride, int same, int precision,
                     float *y_dev) {
    WSC_TRY(check_tensor("wsc_pool_tf_nhwc", ctx, x_dev, y_dev, N, H, W, C, precision));
    WSC_CHECK((k == 2 || k == 3) && (stride == 1 || stride == 2) && stride <= k && (same == 0 || same == 1), WSC_ERR_INVALID,
              "wsc_pool_tf_nhwc: window %d stride %d same %d (window 2 / 3, stride 1 / 2, same 0 / 1)", k, stride, same);
    PoolGeom g;
    WSC_CHECK(pool_geom(same ? POOL_TF_SAME : POOL_TF_VALID, k, stride, 0, false, H, W, &g), WSC_ERR_INVALID,
              "wsc_pool_tf_nhwc: %d x %d x %d x %d is no input of a %d x %d %s window", N, H, W, C, k, k, same ? "SAME" : "VALID");
    return pool_staged(ctx, x_dev, N, H, W, C, g, precision, y_dev);
}

int wsc_pool_same_grad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int C, int avg, int stride,
                            float *dx_dev) {
    WSC_TRY(check_tensor("wsc_pool_same_grad_nhwc", ctx, x_dev, dx_dev, N, H, W, C, WSC_PREC_F32));
    WSC_CHECK(dy_dev != nullptr, WSC_ERR_INVALID, "wsc_pool_same_grad_nhwc: null argument");
    PoolGeom g;
    WSC_CHECK((stride == 1 || stride == 2) && (!avg || stride == 1) && pool_geom(POOL_TF_SAME, 3, stride, 0, avg != 0, H, W, &g),
              WSC_ERR_INVALID, "wsc_pool_same_grad_nhwc: 3x3 max at stride 1 / 2 or 3x3 average at stride 1, got stride %d", stride);
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_pool_grad(ctx, x_dev, dy_dev, N, H, W, C, g, dx_dev);
}

int wsc_pool_tf_grad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int C, int k, int stride, int same,
                          float *dx_dev) {
    WSC_TRY(check_tensor("wsc_pool_tf_grad_nhwc", ctx, x_dev, dx_dev, N, H, W, C, WSC_PREC_F32));
    WSC_CHECK(dy_dev != nullptr, WSC_ERR_INVALID, "wsc_pool_tf_grad_nhwc: null argument");
    WSC_CHECK((k == 2 || k == 3) && (stride == 1 || stride == 2) && stride <= k && (same == 0 || same == 1), WSC_ERR_INVALID,
              "wsc_pool_tf_grad_nhwc: window %d stride %d same %d (window 2 / 3, stride 1 / 2, same 0 / 1)", k, stride, same);
    PoolGeom g;
    WSC_CHECK(pool_geom(same ? POOL_TF_SAME : POOL_TF_VALID, k, stride, 0, false, H, W, &g), WSC_ERR_INVALID,
              "wsc_pool_tf_grad_nhwc: %d x %d x %d x %d is no input of a %d x %d %s window", N, H, W, C, k, k, same ? "SAME" : "VALID");
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_pool_grad(ctx, x_dev, dy_dev, N, H, W, C, g, dx_dev);
}

int wsc_maxpool_grad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int C, int k, int stride, int pad,
                          float *dx_dev) {
    WSC_TRY(check_tensor("wsc_maxpool_grad_nhwc", ctx, x_dev, dx_dev, N, H, W, C, WSC_PREC_F32));
    WSC_CHECK(dy_dev != nullptr, WSC_ERR_INVALID, "wsc_maxpool_grad_nhwc: null argument");
    WSC_CHECK(k >= 1 && stride >= 1 && pad >= 0 && 2 * pad <= k, WSC_ERR_INVALID,
              "wsc_maxpool_grad_nhwc: window %d stride %d padding %d (padding at most half the window)", k, stride, pad);
    PoolGeom g;
    WSC_CHECK(H + 2 * pad >= k && W + 2 * pad >= k && pool_geom(POOL_TORCH, k, stride, pad, false, H, W, &g), WSC_ERR_INVALID,
              "wsc_maxpool_grad_nhwc: a %d x %d map is smaller than the window %d", H, W, k);
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_pool_grad(ctx, x_dev, dy_dev, N, H, W, C, g, dx_dev);
}

} // extern "C"
