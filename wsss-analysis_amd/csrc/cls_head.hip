// cls_head.hip -- 01_train on the device: the loss head of the classifier with the gradient through the head (01_train/demo.py:60-61
// model.compile(loss='binary_crossentropy', metrics=['binary_accuracy', f1]), utilities.py:69-97 f1), and the score side of
// predict(): the ROC thresholds and the thresholded counts (utilities.py:99-165 get_optimal_thresholds,
// get_thresholded_metrics_class, get_thresholded_metrics_overall).  The formulas: include/wsscam.h, wsc_cls_loss,
// wsc_roc_thresholds, wsc_cls_threshold_counts.
//
// wsc_cls_loss.  Inputs are float32; every sum, product, sigmoid and log is double and every output is rounded once.  Every
// floating-point sum has ONE order that depends on the shape alone, and there is no floating-point atomic: two calls give the same
// bits.  The work is a streaming read of the map, a tiny dense stage and a streaming write of grad_feat, all in 16-byte accesses:
//   cls_pool_kernel       grid (chunk, 256-channel tile, sample): 64 column groups of 4 channels x 4 position lanes; a lane adds
//                         (or takes the maximum of, counting the positions that hold it) every 4th position of its chunk in
//                         position order, then the 4 lanes in lane order -> partial [B][S][F] (8 bytes: a double, or {max, count})
//   cls_dense_kernel      one workgroup per sample: the chunks in chunk order -> pooled [F] (LDS and scratch); a wave per class
//                         for the logit (a lane adds its strided float4 columns in order, xor butterfly over the wave), then a
//                         lane per class for sigmoid, loss term, counts and g_l; the sample's loss in class order; g_pooled = sum_c g_l W[c] in class
//                         order -> the share every position (mean) or every maximum (max) receives, float32 [F]
//   cls_finish_kernel     one workgroup: the samples (a thread adds its strided share in order, block_sum) -> loss_dev; grad_bias
//   cls_wgrad_kernel      a thread per (class, 4 channels): the samples in order -> grad_w
//   cls_feat_grad_kernel  the pool kernel's grid: every element of grad_feat written with a float4 store
//
// wsc_roc_thresholds.  One workgroup per class: (descending score bits << 1 | target) as 64-bit keys in LDS, padded with all-ones
// keys to a power of two, bitonic sort; a thread walks a contiguous segment of the sorted keys, integer block scans place the ends
// of the groups of equal scores and then the points the second-difference rule keeps; the first minimum of |tpr - (1 - fpr)| by
// a (value, index) minimum.  Everything but that value is an integer or a copy of a score.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace {

constexpr int CH_MAX_B = 1024;
constexpr int CH_MAX_C = 64;
constexpr int CH_MAX_F = 4096;      // cls_dense_kernel keeps a sample's pooled vector in LDS as doubles (32 KiB at the limit)
constexpr int CH_MAX_N = 65536;
constexpr int CH_THREADS = 256;
constexpr int CH_TILE_F = 256;      // channels of a block of the two streaming kernels: 1 KiB of every position's row
constexpr int CH_LANES = CH_THREADS / (CH_TILE_F / 4); // position lanes of such a block
constexpr int CH_CHUNK = 64;        // positions of a chunk, until there are CH_MAX_CHUNKS of them: the chunking depends on n alone
constexpr int CH_MAX_CHUNKS = 32;
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_DENSE_THREADS = 1024; // cls_dense_kernel: B workgroups are few, so each is wide (16 classes at a time)
enum { CH_PS_LOSS = 0, CH_PS_EQUAL, CH_PS_TP, CH_PS_POSSIBLE, CH_PS_PREDICTED, CH_PS_N }; // per-sample values, [B][CH_PS_N]

// a maximum and the number of positions that hold it, as the 8 bytes of a partial: {count, value bits}
__device__ __forceinline__ double ch_pack(float v, int cnt) {
    return __longlong_as_double(((long long)__float_as_int(v) << 32) | (long long)(unsigned)cnt);
}
__device__ __forceinline__ void ch_unpack(double d, float *v, int *cnt) {
    const long long u = __double_as_longlong(d);
    *v = __int_as_float((int)(u >> 32));
    *cnt = (int)(unsigned)u;
}
__device__ __forceinline__ void ch_max_join(float &mv, int &mc, float v, int cnt) {
    mc = v > mv ? cnt : (v == mv ? mc + cnt : mc);
    mv = max_keep_nan(mv, v); // (a NaN position makes the maximum NaN, as MaxPooling2D's does)
}

// grid (S, ceil(F / CH_TILE_F), B); partial [B][S][F]
template <bool MAXP>
__global__ __launch_bounds__(CH_THREADS) void cls_pool_kernel(const float *__restrict__ feat, int n, int F, int per,
                                                              double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double sh[CH_LANES][CH_TILE_F];
    const int s = blockIdx.x, S = gridDim.x, b = blockIdx.z;
    const int g = threadIdx.x % (CH_TILE_F / 4), lane = threadIdx.x / (CH_TILE_F / 4);
    const int f = blockIdx.y * CH_TILE_F + g * 4; // F is a multiple of 4: the whole float4 is inside, or none of it
    const int p0 = s * per, p1 = min(n, p0 + per);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float mv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int mc[4] = {0, 0, 0, 0};
    if (f < F) {
        const float *src = feat + (size_t)b * n * F + f;
#pragma unroll 4
        for (int p = p0 + lane; p < p1; p += CH_LANES) {
            const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)p * F);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (MAXP) ch_max_join(mv[k], mc[k], e[k] + 0.f, 1); // (-0 counts as +0)
                else acc[k] += (double)e[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[lane][g * 4 + k] = MAXP ? ch_pack(mv[k], mc[k]) : acc[k];
    __syncthreads();
    if (lane == 0 && f < F) {
        double *out = partial + ((size_t)b * S + s) * F + f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (MAXP) {
                float v = mv[k], ov;
                int cnt = mc[k], oc;
                for (int l = 1; l < CH_LANES; ++l) {
                    ch_unpack(sh[l][g * 4 + k], &ov, &oc);
                    ch_max_join(v, cnt, ov, oc);
                }
                out[k] = ch_pack(v, cnt);
            } else {
                double t = acc[k];
                for (int l = 1; l < CH_LANES; ++l) t += sh[l][g * 4 + k];
                out[k] = t;
            }
        }
    }
}

// p = sigmoid(l) and q = sigmoid(-l) = 1 - p, neither through a cancellation
__device__ __forceinline__ void ch_sigmoid(double l, double *p, double *q) {
    const double e = exp(-fabs(l)), big = 1.0 / (1.0 + e), small = e / (1.0 + e);
    *p = l >= 0.0 ? big : small;
    *q = l >= 0.0 ? small : big;
}

// grid (B).  wts [B]: the sample weights; coef [B] = w_b / (C #{w != 0}).
template <bool MAXP>
__global__ __launch_bounds__(CH_DENSE_THREADS) void cls_dense_kernel(const double *__restrict__ partial, int S, int n, int F, int C,
                                                               const float *__restrict__ W, const float *__restrict__ bias,
                                                               const float *__restrict__ target, const double *__restrict__ coef,
                                                               double eps, double hi, double *__restrict__ pooled_out,
                                                               float *__restrict__ score, double *__restrict__ gl_out,
                                                               double *__restrict__ per_sample, float *__restrict__ share_out) {
    __shared__ __attribute__((aligned(16))) double pooled[CH_MAX_F];
    __shared__ int ties[MAXP ? CH_MAX_F : 1];
    __shared__ double gl[CH_MAX_C], term[CH_MAX_C];
    __shared__ int flags[CH_MAX_C]; // bit 0 z == round(p), 1 round(z p), 2 round(z), 3 round(p)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int f = tid; f < F; f += CH_DENSE_THREADS) {
        const double *src = partial + (size_t)b * S * F + f;
        if (MAXP) {
            float v = -INFINITY, ov;
            int cnt = 0, oc;
            for (int s = 0; s < S; ++s) {
                ch_unpack(src[(size_t)s * F], &ov, &oc);
                ch_max_join(v, cnt, ov, oc);
            }
            pooled[f] = (double)v;
            ties[f] = cnt;
        } else {
            double t = 0.0;
            for (int s = 0; s < S; ++s) t += src[(size_t)s * F];
            pooled[f] = t / (double)n;
        }
        pooled_out[(size_t)b * F + f] = pooled[f];
    }
    __syncthreads();
    const double cf = coef[b];
    for (int c = wave; c < C; c += CH_DENSE_THREADS / 64) {
        const float *wr = W + (size_t)c * F;
        double acc = 0.0;
        for (int f = lane * 4; f < F; f += 256) {
            const float4 w = *reinterpret_cast<const float4 *>(wr + f);
            acc += pooled[f] * (double)w.x;
            acc += pooled[f + 1] * (double)w.y;
            acc += pooled[f + 2] * (double)w.z;
            acc += pooled[f + 3] * (double)w.w;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) term[c] = acc; // (the logit without its bias, until the next phase)
    }
    __syncthreads();
    if (tid < C) { // a lane per class: the exp and the two logs of the classes run side by side
        const int c = tid;
        const double l = term[c] + (bias ? (double)bias[c] : 0.0), z = (double)target[(size_t)b * C + c];
        double p, q;
        ch_sigmoid(l, &p, &q);
        // (a NaN score stays NaN through the clip, as K.clip's does: fmin / fmax would return the bound, a finite loss and a zero
        // gradient for a diverged model)
        const bool nan = p != p;
        const double pc = nan ? p : fmin(fmax(p, eps), hi), qc = nan ? p : fmin(fmax(q, 1.0 - hi), 1.0 - eps); // qc = 1 - pc
        term[c] = -(z * log(pc) + (1.0 - z) * log(qc));
        gl[c] = nan ? p : ((p >= eps && p <= hi) ? cf * (p - z) + 0.0 : 0.0); // (+ 0.0: a zero weight gives +0.0 too, never -0.0)
        const double rp = rint(p); // half to even: 0.5 -> 0
        // (a NaN score has no rounding: it counts as neither equal, true positive nor predicted -- NaN != 0.0 is true)
        flags[c] = nan ? (rint(z) != 0.0 ? 4 : 0) : (z == rp ? 1 : 0) | (rint(z * p) != 0.0 ? 2 : 0) | (rint(z) != 0.0 ? 4 : 0) | (rp != 0.0 ? 8 : 0);
        if (score) score[(size_t)b * C + c] = (float)p;
        gl_out[(size_t)b * C + c] = gl[c];
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0, cnt[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < C; ++c) {
            t += term[c];
            for (int k = 0; k < 4; ++k) cnt[k] += (double)((flags[c] >> k) & 1);
        }
        double *o = per_sample + (size_t)b * CH_PS_N;
        o[CH_PS_LOSS] = t / (double)C;
        for (int k = 0; k < 4; ++k) o[CH_PS_EQUAL + k] = cnt[k];
    }
    if (share_out)
        for (int f = tid * 4; f < F; f += CH_DENSE_THREADS * 4) {
            double g[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < C; ++c) {
                const float4 w = *reinterpret_cast<const float4 *>(W + (size_t)c * F + f);
                const double d = gl[c];
                g[0] += d * (double)w.x;
                g[1] += d * (double)w.y;
                g[2] += d * (double)w.z;
                g[3] += d * (double)w.w;
            }
            float4 o;
            o.x = (float)(g[0] / (double)(MAXP ? ties[f] : n));
            o.y = (float)(g[1] / (double)(MAXP ? ties[f + 1] : n));
            o.z = (float)(g[2] / (double)(MAXP ? ties[f + 2] : n));
            o.w = (float)(g[3] / (double)(MAXP ? ties[f + 3] : n));
            *reinterpret_cast<float4 *>(share_out + (size_t)b * F + f) = o;
        }
}

// one workgroup
__global__ __launch_bounds__(CH_THREADS) void cls_finish_kernel(const double *__restrict__ per_sample, const double *__restrict__ wts,
                                                                const double *__restrict__ gl, int B, int C, double nz,
                                                                double *__restrict__ loss, float *__restrict__ grad_bias) {
    __shared__ double scratch[CH_WAVES * 6];
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // sum w l, sum l, the four counts
    for (int b = threadIdx.x; b < B; b += CH_THREADS) {
        const double *p = per_sample + (size_t)b * CH_PS_N;
        v[0] += wts[b] * p[CH_PS_LOSS];
        v[1] += p[CH_PS_LOSS];
        for (int k = 0; k < 4; ++k) v[2 + k] += p[CH_PS_EQUAL + k];
    }
    block_sum<6>(v, scratch);
    if (threadIdx.x == 0) {
        loss[WSC_CLS_LOSS_TOTAL] = v[0] / nz;
        loss[WSC_CLS_LOSS_MEAN] = v[1] / (double)B;
        loss[WSC_CLS_LOSS_N_EQUAL] = v[2];
        loss[WSC_CLS_LOSS_TP] = v[3];
        loss[WSC_CLS_LOSS_POSSIBLE] = v[4];
        loss[WSC_CLS_LOSS_PREDICTED] = v[5];
    }
    if (grad_bias && threadIdx.x < C) {
        double t = 0.0;
        for (int b = 0; b < B; ++b) t += gl[(size_t)b * C + threadIdx.x];
        grad_bias[threadIdx.x] = (float)t;
    }
}

// grid (ceil(F / 4 / CH_THREADS), C)
__global__ __launch_bounds__(CH_THREADS) void cls_wgrad_kernel(const double *__restrict__ gl, const double *__restrict__ pooled, int B,
                                                               int F, int C, float *__restrict__ grad_w) {
    const int f = (blockIdx.x * CH_THREADS + threadIdx.x) * 4, c = blockIdx.y;
    if (f >= F) return;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b) {
        const double d = gl[(size_t)b * C + c];
        const double2 a = *reinterpret_cast<const double2 *>(pooled + (size_t)b * F + f);
        const double2 e = *reinterpret_cast<const double2 *>(pooled + (size_t)b * F + f + 2);
        g[0] += d * a.x;
        g[1] += d * a.y;
        g[2] += d * e.x;
        g[3] += d * e.y;
    }
    float4 o;
    o.x = (float)g[0];
    o.y = (float)g[1];
    o.z = (float)g[2];
    o.w = (float)g[3];
    *reinterpret_cast<float4 *>(grad_w + (size_t)c * F + f) = o;
}

// grid (S, ceil(F / CH_TILE_F), B): every element of grad_feat
template <bool MAXP>
__global__ __launch_bounds__(CH_THREADS) void cls_feat_grad_kernel(const float *__restrict__ feat, const double *__restrict__ pooled,
                                                                   const float *__restrict__ share, int n, int F, int per,
                                                                   float *__restrict__ grad_feat) {
    const int s = blockIdx.x, b = blockIdx.z;
    const int g = threadIdx.x % (CH_TILE_F / 4), lane = threadIdx.x / (CH_TILE_F / 4);
    const int f = blockIdx.y * CH_TILE_F + g * 4;
    if (f >= F) return;
    const int p0 = s * per, p1 = min(n, p0 + per);
    const float4 sh = *reinterpret_cast<const float4 *>(share + (size_t)b * F + f);
    float mx[4] = {0.f, 0.f, 0.f, 0.f};
    if (MAXP) {
#pragma unroll
        for (int k = 0; k < 4; ++k) mx[k] = (float)pooled[(size_t)b * F + f + k]; // (a float32 value: the conversion is exact)
    }
    const size_t base = (size_t)b * n * F + f;
#pragma unroll 4
    for (int p = p0 + lane; p < p1; p += CH_LANES) {
        float4 o = sh;
        if (MAXP) {
            const float4 v = *reinterpret_cast<const float4 *>(feat + base + (size_t)p * F);
            o.x = v.x + 0.f == mx[0] ? sh.x : 0.f;
            o.y = v.y + 0.f == mx[1] ? sh.y : 0.f;
            o.z = v.z + 0.f == mx[2] ? sh.z : 0.f;
            o.w = v.w + 0.f == mx[3] ? sh.w : 0.f;
        }
        *reinterpret_cast<float4 *>(grad_feat + base + (size_t)p * F) = o;
    }
}

template <bool MAXP>
int cls_loss_launch(wsc_ctx *ctx, const float *feat, int B, int n, int F, const float *w, const float *bias, int C, const float *target,
                    const std::vector<double> &wts, double nz, double *loss, float *score, float *g_feat, float *g_w, float *g_bias) {
    const int S = std::min(CH_MAX_CHUNKS, (n + CH_CHUNK - 1) / CH_CHUNK), per = (n + S - 1) / S;
    const int tiles = (F + CH_TILE_F - 1) / CH_TILE_F;
    // scratch of the call: [partial | pooled | g_l | per-sample values | share]
    const auto whole16 = [](size_t bytes) { return (bytes + 15) / 16 * 16; }; // the sections start 16-byte aligned
    const size_t partial_bytes = (size_t)B * S * F * sizeof(double), pooled_bytes = (size_t)B * F * sizeof(double);
    const size_t gl_bytes = whole16((size_t)B * C * sizeof(double)), ps_bytes = whole16((size_t)B * CH_PS_N * sizeof(double));
    const size_t share_bytes = g_feat ? (size_t)B * F * sizeof(float) : 0;
    char *scratch = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, partial_bytes + pooled_bytes + gl_bytes + ps_bytes + share_bytes, (void **)&scratch));
    WscCachedGuard scratch_guard(ctx, scratch);
    double *partial = (double *)scratch, *pooled = (double *)(scratch + partial_bytes);
    double *gl = (double *)(scratch + partial_bytes + pooled_bytes), *per_sample = (double *)(scratch + partial_bytes + pooled_bytes + gl_bytes);
    float *share = g_feat ? (float *)(scratch + partial_bytes + pooled_bytes + gl_bytes + ps_bytes) : nullptr;
    std::vector<double> coef(B);
    for (int b = 0; b < B; ++b) coef[b] = wts[b] / ((double)C * nz);
    WscStagedTable tab(ctx);
    const size_t wts_at = tab.add(wts), coef_at = tab.add(coef);
    WSC_TRY(tab.upload());
    const float eps = 1e-7f, hi = 1.0f - eps; // K.epsilon() and 1 - K.epsilon() as float32
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * n * F * 4.0 * (1.0 + (g_feat ? (MAXP ? 2.0 : 1.0) : 0.0)));
    hipLaunchKernelGGL(cls_pool_kernel<MAXP>, dim3(S, tiles, B), dim3(CH_THREADS), 0, ctx->stream, feat, n, F, per, partial);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(cls_dense_kernel<MAXP>, dim3(B), dim3(CH_DENSE_THREADS), 0, ctx->stream, (const double *)partial, S, n, F, C, w, bias,
                       target, tab.at<const double>(coef_at), (double)eps, (double)hi, pooled, score, gl, per_sample, share);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(cls_finish_kernel, dim3(1), dim3(CH_THREADS), 0, ctx->stream, (const double *)per_sample,
                       tab.at<const double>(wts_at), (const double *)gl, B, C, nz, loss, g_bias);
    WSC_HIP(hipGetLastError());
    if (g_w) {
        hipLaunchKernelGGL(cls_wgrad_kernel, dim3((F / 4 + CH_THREADS - 1) / CH_THREADS, C), dim3(CH_THREADS), 0, ctx->stream,
                           (const double *)gl, (const double *)pooled, B, F, C, g_w);
        WSC_HIP(hipGetLastError());
    }
    if (g_feat) {
        hipLaunchKernelGGL(cls_feat_grad_kernel<MAXP>, dim3(S, tiles, B), dim3(CH_THREADS), 0, ctx->stream, feat, (const double *)pooled,
                           (const float *)share, n, F, per, g_feat);
        WSC_HIP(hipGetLastError());
    }
    tab.release(); // stream-ordered reuse, as the scratch block
    scratch_guard.free_now();
    return WSC_OK;
}

bool ch_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
bool ch_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// ---- ROC ------------------------------------------------------------------------------------------------------------------------
constexpr int ROC_MAX_N = 16384; // a class is sorted in LDS: 128 KiB of keys at the limit
constexpr int ROC_MAX_C = 64;
constexpr int ROC_THREADS = 1024;
constexpr int ROC_WAVES = ROC_THREADS / 64;
constexpr size_t ROC_TAIL_BYTES = 64 * sizeof(int) + ROC_WAVES * (sizeof(double) + sizeof(int)); // behind the keys

// the exclusive prefix of v over the threads of the workgroup and the total, integers; scratch: ROC_WAVES ints
__device__ __forceinline__ int roc_scan(int v, int *scratch, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __syncthreads(); // (an earlier call's readers are done with scratch)
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < ROC_WAVES; ++w) {
        const int s = scratch[w];
        base += w < wave ? s : 0;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// grid (C).  LDS: uint64 key[P], then ROC_TAIL_BYTES.  groups [C][3][N] (fps, tps, score bits of every group of equal scores),
// curve [C][3][N + 1] (the kept points).
__global__ __launch_bounds__(ROC_THREADS) void roc_kernel(const float *__restrict__ score, const float *__restrict__ target, int N, int C,
                                                          int P, int *__restrict__ groups, int *__restrict__ curve,
                                                          float *__restrict__ thresh, int *__restrict__ status,
                                                          int *__restrict__ n_points, int *__restrict__ fps_out,
                                                          int *__restrict__ tps_out) {
    extern __shared__ __attribute__((aligned(16))) char roc_lds[];
    unsigned long long *key = (unsigned long long *)roc_lds;
    int *scan = (int *)(key + P);                // 64 ints (ROC_WAVES used)
    double *best_v = (double *)(scan + 64);      // ROC_WAVES
    int *best_j = (int *)(best_v + ROC_WAVES);   // ROC_WAVES
    const int c = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < P; i += ROC_THREADS) {
        unsigned long long k = ~0ull; // padding sorts last
        if (i < N) {
            const unsigned long long desc = (uint32_t)~float_order_bits(score[(size_t)i * C + c]);
            k = (desc << 1) | (target[(size_t)i * C + c] == 1.f ? 1ull : 0ull);
        }
        key[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += ROC_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j; // both < P
                const unsigned long long a = key[lo], d = key[hi];
                if ((a > d) == ((lo & k) == 0)) {
                    key[lo] = d;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    // the groups of equal scores: a thread walks keys [i0, i1)
    int *g_fps = groups + (size_t)c * 3 * N, *g_tps = g_fps + N, *g_bits = g_tps + N;
    int *k_fps = curve + (size_t)c * 3 * (N + 1), *k_tps = k_fps + (N + 1), *k_bits = k_tps + (N + 1);
    const int per = (N + ROC_THREADS - 1) / ROC_THREADS, i0 = min(N, tid * per), i1 = min(N, i0 + per);
    int pos = 0, ends = 0;
    for (int i = i0; i < i1; ++i) {
        pos += (int)(key[i] & 1);
        ends += (i == N - 1 || (key[i] >> 1) != (key[i + 1] >> 1)) ? 1 : 0;
    }
    int total_pos, m;
    int tps = roc_scan(pos, scan, &total_pos), at = roc_scan(ends, scan, &m);
    for (int i = i0; i < i1; ++i) {
        tps += (int)(key[i] & 1);
        if (i == N - 1 || (key[i] >> 1) != (key[i + 1] >> 1)) { // at < m <= N
            g_fps[at] = i + 1 - tps;
            g_tps[at] = tps;
            g_bits[at] = (int)~(uint32_t)(key[i] >> 1);
            ++at;
        }
    }
    __syncthreads(); // (the workgroup's own stores to `groups` are visible to its loads)
    // drop interior point i when both second differences are 0, THEN prepend (0, 0, +inf)
    const int per_m = (m + ROC_THREADS - 1) / ROC_THREADS, j0 = min(m, tid * per_m), j1 = min(m, j0 + per_m);
    int kept = 0;
    for (int j = j0; j < j1; ++j)
        kept += (j == 0 || j == m - 1 || g_fps[j - 1] - 2 * g_fps[j] + g_fps[j + 1] != 0 || g_tps[j - 1] - 2 * g_tps[j] + g_tps[j + 1] != 0) ? 1 : 0;
    int K;
    int out = 1 + roc_scan(kept, scan, &K);
    K += 1; // <= N + 1
    for (int j = j0; j < j1; ++j)
        if (j == 0 || j == m - 1 || g_fps[j - 1] - 2 * g_fps[j] + g_fps[j + 1] != 0 || g_tps[j - 1] - 2 * g_tps[j] + g_tps[j + 1] != 0) {
            k_fps[out] = g_fps[j];
            k_tps[out] = g_tps[j];
            k_bits[out] = g_bits[j];
            ++out;
        }
    if (tid == 0) {
        k_fps[0] = 0;
        k_tps[0] = 0;
        k_bits[0] = (int)float_order_bits(INFINITY);
    }
    __syncthreads();
    const int n_pos = total_pos, n_neg = N - total_pos;
    if (fps_out)
        for (int j = tid; j < N + 1; j += ROC_THREADS) {
            fps_out[(size_t)c * (N + 1) + j] = j < K ? k_fps[j] : 0;
            tps_out[(size_t)c * (N + 1) + j] = j < K ? k_tps[j] : 0;
        }
    // the FIRST minimum of |tpr - (1 - fpr)|
    double bv = INFINITY;
    int bj = 0x7fffffff;
    if (n_pos > 0 && n_neg > 0)
        for (int j = tid; j < K; j += ROC_THREADS) {
            const double tpr = (double)k_tps[j] / (double)n_pos, fpr = (double)k_fps[j] / (double)n_neg;
            const double v = fabs(tpr - (1.0 - fpr));
            if (v < bv) { // (j ascends: the first of equal values stays)
                bv = v;
                bj = j;
            }
        }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oj = __shfl_xor(bj, off, 64);
        if (ov < bv || (ov == bv && oj < bj)) {
            bv = ov;
            bj = oj;
        }
    }
    if ((tid & 63) == 0) {
        best_v[tid >> 6] = bv;
        best_j[tid >> 6] = bj;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ROC_WAVES; ++w)
            if (best_v[w] < bv || (best_v[w] == bv && best_j[w] < bj)) {
                bv = best_v[w];
                bj = best_j[w];
            }
        const bool degenerate = n_pos == 0 || n_neg == 0;
        thresh[c] = degenerate ? INFINITY : float_from_order_bits((uint32_t)k_bits[bj]); // bj < K
        status[c] = (n_pos == 0 ? WSC_ROC_NO_POSITIVE : 0) | (n_neg == 0 ? WSC_ROC_NO_NEGATIVE : 0);
        if (n_points) n_points[c] = K;
    }
}

constexpr int TC_THREADS = 256;
constexpr int TC_PER_BLOCK = TC_THREADS * 16; // elements of a block

// grid (ceil(N C / TC_PER_BLOCK)); counts [C][WSC_CLS_COUNT_N], zeroed before the launch.  Integer atomics: exact in any order.
__global__ __launch_bounds__(TC_THREADS) void cls_threshold_counts_kernel(const float *__restrict__ score, const float *__restrict__ target,
                                                                          const float *__restrict__ thresh, long long total, int C,
                                                                          unsigned long long *__restrict__ counts) {
    __shared__ unsigned local[ROC_MAX_C * WSC_CLS_COUNT_N];
    for (int i = threadIdx.x; i < C * WSC_CLS_COUNT_N; i += TC_THREADS) local[i] = 0;
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * TC_PER_BLOCK, e1 = min(total, e0 + TC_PER_BLOCK);
    for (long long e = e0 + threadIdx.x; e < e1; e += TC_THREADS) {
        const int c = (int)(e % C);
        const float z = target[e];
        const bool pred = score[e] >= thresh[c];
        int slot = -1;
        if (z == 1.f) slot = pred ? WSC_CLS_COUNT_TP : WSC_CLS_COUNT_FN;
        else if (z == 0.f) slot = pred ? WSC_CLS_COUNT_FP : WSC_CLS_COUNT_TN;
        if (slot >= 0) atomicAdd(&local[c * WSC_CLS_COUNT_N + slot], 1u);
        if (z == (pred ? 1.f : 0.f)) atomicAdd(&local[c * WSC_CLS_COUNT_N + WSC_CLS_COUNT_EQUAL], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * WSC_CLS_COUNT_N; i += TC_THREADS)
        if (local[i]) atomicAdd(&counts[i], (unsigned long long)local[i]);
}

__global__ __launch_bounds__(256) void cls_copy_kernel(const float *__restrict__ src, long long n, float *__restrict__ dst) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

} // namespace

extern "C" {

int wsc_cls_loss(wsc_ctx *ctx, const float *feat_dev, int B, int n, int F, int pool, const float *w_dev, const float *bias_dev, int C,
                 const float *target_dev, const float *sample_w_host, double *loss_dev, float *score_dev, float *grad_feat_dev,
                 float *grad_w_dev, float *grad_bias_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_cls_loss: ctx is NULL");
    WSC_CHECK(pool == WSC_CLS_POOL_MEAN || pool == WSC_CLS_POOL_MAX, WSC_ERR_INVALID, "wsc_cls_loss: pool=%d (0: mean, 1: max)", pool);
    WSC_CHECK(feat_dev, WSC_ERR_INVALID, "wsc_cls_loss: feat_dev is NULL");
    WSC_CHECK(w_dev, WSC_ERR_INVALID, "wsc_cls_loss: w_dev is NULL");
    WSC_CHECK(target_dev, WSC_ERR_INVALID, "wsc_cls_loss: target_dev is NULL");
    WSC_CHECK(loss_dev, WSC_ERR_INVALID, "wsc_cls_loss: loss_dev is NULL");
    WSC_CHECK(B >= 1 && B <= CH_MAX_B, WSC_ERR_INVALID, "wsc_cls_loss: B=%d (1 <= B <= %d)", B, CH_MAX_B);
    WSC_CHECK(C >= 1 && C <= CH_MAX_C, WSC_ERR_INVALID, "wsc_cls_loss: C=%d (1 <= C <= %d)", C, CH_MAX_C);
    WSC_CHECK(F >= 4 && F <= CH_MAX_F && F % 4 == 0, WSC_ERR_INVALID, "wsc_cls_loss: F=%d (a multiple of 4, 4 <= F <= %d)", F, CH_MAX_F);
    WSC_CHECK(n >= 1 && n <= CH_MAX_N, WSC_ERR_INVALID, "wsc_cls_loss: n=%d (1 <= n <= %d)", n, CH_MAX_N);
    WSC_CHECK(ch_aligned16(feat_dev) && ch_aligned16(w_dev) && ch_aligned16(grad_feat_dev) && ch_aligned16(grad_w_dev), WSC_ERR_INVALID,
              "wsc_cls_loss: feat_dev, w_dev, grad_feat_dev and grad_w_dev are read and written 16 bytes at a time: one is not aligned");
    std::vector<double> wts(B, 1.0);
    double nz = 0.0;
    for (int b = 0; b < B; ++b) {
        if (sample_w_host) {
            const float w = sample_w_host[b];
            WSC_CHECK(std::isfinite(w) && w >= 0.f, WSC_ERR_INVALID, "wsc_cls_loss: sample_w_host[%d]=%g (finite and >= 0)", b, (double)w);
            wts[b] = (double)w;
        }
        nz += wts[b] != 0.0 ? 1.0 : 0.0;
    }
    WSC_CHECK(nz > 0.0, WSC_ERR_INVALID, "wsc_cls_loss: sample_w_host has no non-zero weight (the loss divides by their number)");
    const size_t feat_bytes = (size_t)B * n * F * 4, w_bytes = (size_t)C * F * 4, bc_bytes = (size_t)B * C * 4;
    const struct { const void *p; size_t bytes; const char *name; } in[] = {{feat_dev, feat_bytes, "feat_dev"}, {w_dev, w_bytes, "w_dev"},
        {bias_dev, (size_t)C * 4, "bias_dev"}, {target_dev, bc_bytes, "target_dev"}},
        out[] = {{loss_dev, WSC_CLS_LOSS_N * sizeof(double), "loss_dev"}, {score_dev, bc_bytes, "score_dev"},
                 {grad_feat_dev, feat_bytes, "grad_feat_dev"}, {grad_w_dev, w_bytes, "grad_w_dev"}, {grad_bias_dev, (size_t)C * 4, "grad_bias_dev"}};
    for (size_t o = 0; o < sizeof(out) / sizeof(out[0]); ++o) {
        for (const auto &i : in)
            WSC_CHECK(!ch_overlap(out[o].p, out[o].bytes, i.p, i.bytes), WSC_ERR_INVALID, "wsc_cls_loss: %s overlaps %s", out[o].name, i.name);
        for (size_t q = o + 1; q < sizeof(out) / sizeof(out[0]); ++q)
            WSC_CHECK(!ch_overlap(out[o].p, out[o].bytes, out[q].p, out[q].bytes), WSC_ERR_INVALID, "wsc_cls_loss: %s overlaps %s",
                      out[o].name, out[q].name);
    }
    WSC_HIP(hipSetDevice(ctx->device));
    if (pool == WSC_CLS_POOL_MAX)
        return cls_loss_launch<true>(ctx, feat_dev, B, n, F, w_dev, bias_dev, C, target_dev, wts, nz, loss_dev, score_dev, grad_feat_dev,
                                     grad_w_dev, grad_bias_dev);
    return cls_loss_launch<false>(ctx, feat_dev, B, n, F, w_dev, bias_dev, C, target_dev, wts, nz, loss_dev, score_dev, grad_feat_dev,
                                  grad_w_dev, grad_bias_dev);
}

int wsc_roc_thresholds(wsc_ctx *ctx, const float *score_dev, const float *target_dev, int N, int C, float *thresh_dev, int32_t *status_dev,
                       int32_t *n_points_dev, int32_t *fps_dev, int32_t *tps_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_roc_thresholds: ctx is NULL");
    WSC_CHECK(score_dev, WSC_ERR_INVALID, "wsc_roc_thresholds: score_dev is NULL");
    WSC_CHECK(target_dev, WSC_ERR_INVALID, "wsc_roc_thresholds: target_dev is NULL");
    WSC_CHECK(thresh_dev, WSC_ERR_INVALID, "wsc_roc_thresholds: thresh_dev is NULL");
    WSC_CHECK(status_dev, WSC_ERR_INVALID, "wsc_roc_thresholds: status_dev is NULL");
    WSC_CHECK(N >= 1 && N <= ROC_MAX_N, WSC_ERR_INVALID, "wsc_roc_thresholds: N=%d (1 <= N <= %d: a class is sorted in LDS)", N, ROC_MAX_N);
    WSC_CHECK(C >= 1 && C <= ROC_MAX_C, WSC_ERR_INVALID, "wsc_roc_thresholds: C=%d (1 <= C <= %d)", C, ROC_MAX_C);
    WSC_CHECK((fps_dev == nullptr) == (tps_dev == nullptr), WSC_ERR_INVALID, "wsc_roc_thresholds: fps_dev and tps_dev come together");
    WSC_HIP(hipSetDevice(ctx->device));
    int P = 1;
    while (P < N) P <<= 1;
    const size_t groups_bytes = (size_t)C * 3 * N * sizeof(int), curve_bytes = (size_t)C * 3 * (N + 1) * sizeof(int);
    char *scratch = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, groups_bytes + curve_bytes, (void **)&scratch));
    WscCachedGuard scratch_guard(ctx, scratch);
    const size_t lds = (size_t)P * sizeof(unsigned long long) + ROC_TAIL_BYTES;
    // beyond the 64 KiB a launch gets by default the limit is raised first, and a refusal ends the call.  Raised to what the
    // LARGEST class needs, whatever this call's size: wsc_set_max_dynamic_lds sets a kernel's limit once per device, and two
    // sizes lie beyond 64 KiB (P = 8192 and P = 16384)
    if (lds > 64 * 1024)
        WSC_TRY(wsc_set_max_dynamic_lds(ctx, reinterpret_cast<const void *>(roc_kernel),
                                        (int)(ROC_MAX_N * sizeof(unsigned long long) + ROC_TAIL_BYTES)));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)N * C * 8.0);
    hipLaunchKernelGGL(roc_kernel, dim3(C), dim3(ROC_THREADS), lds, ctx->stream, score_dev, target_dev, N, C, P, (int *)scratch,
                       (int *)(scratch + groups_bytes), thresh_dev, status_dev, n_points_dev, fps_dev, tps_dev);
    WSC_HIP(hipGetLastError());
    scratch_guard.free_now();
    return WSC_OK;
}

int wsc_cls_threshold_counts(wsc_ctx *ctx, const float *score_dev, const float *target_dev, int N, int C, const float *thresh_dev,
                             int64_t *counts_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_cls_threshold_counts: ctx is NULL");
    WSC_CHECK(score_dev, WSC_ERR_INVALID, "wsc_cls_threshold_counts: score_dev is NULL");
    WSC_CHECK(target_dev, WSC_ERR_INVALID, "wsc_cls_threshold_counts: target_dev is NULL");
    WSC_CHECK(thresh_dev, WSC_ERR_INVALID, "wsc_cls_threshold_counts: thresh_dev is NULL");
    WSC_CHECK(counts_dev, WSC_ERR_INVALID, "wsc_cls_threshold_counts: counts_dev is NULL");
    WSC_CHECK(N >= 1 && N <= ROC_MAX_N, WSC_ERR_INVALID, "wsc_cls_threshold_counts: N=%d (1 <= N <= %d)", N, ROC_MAX_N);
    WSC_CHECK(C >= 1 && C <= ROC_MAX_C, WSC_ERR_INVALID, "wsc_cls_threshold_counts: C=%d (1 <= C <= %d)", C, ROC_MAX_C);
    WSC_HIP(hipSetDevice(ctx->device));
    const long long total = (long long)N * C;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)total * 8.0);
    WSC_HIP(hipMemsetAsync(counts_dev, 0, (size_t)C * WSC_CLS_COUNT_N * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(cls_threshold_counts_kernel, dim3((unsigned)((total + TC_PER_BLOCK - 1) / TC_PER_BLOCK)), dim3(TC_THREADS), 0,
                       ctx->stream, score_dev, target_dev, thresh_dev, total, C, (unsigned long long *)counts_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int wsc_cls_scores_append(wsc_ctx *ctx, const float *src_dev, long long elems, float *dst_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_cls_scores_append: ctx is NULL");
    WSC_CHECK(elems >= 0 && (elems == 0 || (src_dev && dst_dev)), WSC_ERR_INVALID, "wsc_cls_scores_append: elems=%lld, or a NULL buffer", elems);
    if (elems == 0) return WSC_OK;
    WSC_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(cls_copy_kernel, dim3(wsc_grid_for(elems)), dim3(256), 0, ctx->stream, src_dev, elems, dst_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

} // extern "C"
