// seg_loss.hip -- the SEC / DSRG training losses and the gradient they send into fc8 (03a_sec-dsrg/SEC.py:363-465 getloss,
// get_seed_loss, get_expand_loss, get_constrain_loss; DSRG.py:459-518 getloss, get_balanced_seed_loss, get_constrain_loss; the
// chain rule through build_sp_softmax, SEC.py:246-249).  The formulas: include/wsscam.h, wsc_seg_loss.
//
// Inputs are float32; every log, exp, product and sum is double and every output is rounded once.  Every sum has ONE order,
// whatever the launch: a thread adds its strided share in index order, block_sum adds the threads (xor butterfly inside a wave,
// then the waves in wave order).  No floating-point atomic anywhere: two calls on one input give the same bits.
//
//   seg_loss_rank_kernel    SEC, one workgroup per (class, image), background included: the map with its pixel indices as 64-bit
//                           keys (order-preserving value bits << 32 | pixel) in LDS, padded with all-ones keys to a power of two,
//                           bitonic sort ascending -- equal values keep pixel order, the tie rule of np.argsort(kind='stable').
//                           Leaves each pixel's rank (uint16 plane [B][C][n]) and the map's rank-weighted mean, maximum and the
//                           number of pixels at the maximum.
//   seg_loss_pixel_kernel   the sums of the seed and constrain terms and the cue counts of one slice of an image (up to 16 slices of
//                           at least 2048 elements; the slicing depends on the shape alone).  One workgroup per image took 82 us at
//                           16 x 41 x 41 x 21 and was the longest kernel of the call (profiles/README.md).
//   seg_loss_finish_kernel  one workgroup, a thread per image: the slices in slice order, (SEC) the image's three expand terms
//                           from the map statistics; then the means over the batch -> loss_dev
//   seg_loss_grad_kernel    one thread per pixel: dL/dp of every class (registers), <dL/dp, s>, then dL/dp and / or dL/dfc8.
//                           Writes every element, plain zeros included.
// The compare-exchange steps of stride j < 32 touch keys 16 j bytes apart (a 2 j-way conflict of the 8-byte accesses at j = 1);
// at the reference's size the sort is 66 steps of two keys per thread with a barrier each, 36 us for 16 x 21 maps.
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int SL_MAX_C = 32;         // classes: the gradient kernel keeps dL/dp of a pixel in registers (wsc_dsrg_seed_grow's bound)
constexpr int SL_MAX_PIXELS = 8192;  // H * W: the keys of a map live in LDS, 64 KiB at the limit (wsc_dsrg_seed_grow's bound)
constexpr int SL_SORT_THREADS = 512;
constexpr int SL_PIXEL_THREADS = 256;
constexpr int SL_PIXEL_ELEMS = 2048;  // elements of a slice of the per-pixel sums: a slice count depends on the shape alone
constexpr int SL_MAX_SLICES = 16;
constexpr int SL_GRAD_THREADS = 128;
constexpr int SL_FINISH_THREADS = 256;
constexpr int SL_MAX_WAVES = SL_SORT_THREADS / 64; // the widest workgroup that calls block_sum

struct SlMapStat { // one (image, class) map after the sort
    double mean;   // sum_i sorted_i w_i / Z
    double vmax;   // the maximum over the pixels
    double log_mean, log_rest; // log(mean), log(1 - vmax): taken here, one map per workgroup, not in the finish kernel's class loop
    int ties;      // pixels at the maximum (TensorFlow's reduce_max gradient splits among them)
    int pad;
};
// per-image sums, [B][SL_P_N]
enum { SL_P_SEED_BG = 0, SL_P_SEED_FG, SL_P_CNT_BG, SL_P_CNT_FG, SL_P_CONSTRAIN, SL_P_L1, SL_P_L2, SL_P_L3, SL_P_N };

// (block_sum, the workgroup sum every kernel here ends in: common.h; scratch: SL_MAX_WAVES * NV doubles)

// (float_order_bits / float_from_order_bits, the order-preserving key of a value: common.h)

// grid (C, B).  LDS: uint64 key[P], then block_sum's scratch.
__global__ __launch_bounds__(SL_SORT_THREADS) void seg_loss_rank_kernel(const float *__restrict__ prob, int n, int P, int C,
                                                                         const float *__restrict__ w_fg, const float *__restrict__ w_bg,
                                                                         double z_fg, double z_bg, uint16_t *__restrict__ rank,
                                                                         SlMapStat *__restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) char sl_lds[];
    unsigned long long *key = (unsigned long long *)sl_lds;
    double *scratch = (double *)(key + P);
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *src = prob + (size_t)b * n * C + c;
    for (int i = tid; i < P; i += SL_SORT_THREADS)
        key[i] = i < n ? ((unsigned long long)float_order_bits(src[(size_t)i * C]) << 32) | (unsigned)i : ~0ull; // padding sorts last
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += SL_SORT_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j; // both < P
                const unsigned long long a = key[lo], d = key[hi];
                if ((a > d) == ((lo & k) == 0)) {
                    key[lo] = d;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    const float *w = c ? w_fg : w_bg;
    const uint32_t top = (uint32_t)(key[n - 1] >> 32);
    uint16_t *r = rank + ((size_t)b * C + c) * n;
    double acc[2] = {0.0, 0.0}; // sum sorted_i w_i, pixels at the maximum
    for (int i = tid; i < n; i += SL_SORT_THREADS) {
        const unsigned long long k = key[i];
        const uint32_t bits = (uint32_t)(k >> 32);
        r[(uint32_t)k] = (uint16_t)i; // (uint32_t)k < n: a pixel index
        acc[0] += (double)float_from_order_bits(bits) * (double)w[i];
        acc[1] += bits == top ? 1.0 : 0.0;
    }
    block_sum<2>(acc, scratch);
    if (tid == 0) {
        SlMapStat s;
        s.mean = acc[0] / (c ? z_fg : z_bg);
        s.vmax = (double)float_from_order_bits(top);
        s.log_mean = log(s.mean);
        s.log_rest = log(1.0 - s.vmax);
        s.ties = (int)acc[1];
        s.pad = 0;
        stat[(size_t)b * C + c] = s;
    }
}

// stat = labels[:, 1:] > 0: the image's number of positive foreground classes
__device__ __forceinline__ double sl_positives(const float *__restrict__ lab, int C) {
    double s = 0.0;
    for (int c = 1; c < C; ++c) s += lab[c] > 0.f ? 1.0 : 0.0;
    return s;
}

// grid (S, B): slice s of image b's n * C elements.  LDS: block_sum's scratch.  chunk [B][S][SL_P_CONSTRAIN + 1].
template <bool DSRG>
__global__ __launch_bounds__(SL_PIXEL_THREADS) void seg_loss_pixel_kernel(const float *__restrict__ prob, const float *__restrict__ crf,
                                                                           const float *__restrict__ cues, int n, int C,
                                                                           double *__restrict__ chunk) {
    extern __shared__ __attribute__((aligned(16))) char sl_lds[];
    double *scratch = (double *)sl_lds;
    const int b = blockIdx.y, S = gridDim.x, tid = threadIdx.x, total = n * C; // <= 8192 * 32
    const int per = (total + S - 1) / S, e0 = blockIdx.x * per, e1 = min(total, e0 + per);
    const size_t base = (size_t)b * total;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0}; // SL_P_SEED_BG .. SL_P_CONSTRAIN
    for (int e = e0 + tid; e < e1; e += SL_PIXEL_THREADS) {
        const double p = (double)prob[base + e], q = exp((double)crf[base + e]);
        const float cue = cues[base + e];
        if (cue != 0.f) { // (a zero cue adds 0 to both sums: probabilities are > 0)
            const int fg = (e % C) > 0;
            v[SL_P_SEED_BG + fg] += (double)cue * log(p);
            v[SL_P_CNT_BG + fg] += (double)cue;
        }
        v[SL_P_CONSTRAIN] += DSRG ? q * log(q / (p + 1e-8) + 1e-8) : q * log(q / p);
    }
    block_sum<5>(v, scratch);
    if (tid == 0) {
        double *o = chunk + ((size_t)b * S + blockIdx.x) * 5;
        for (int k = 0; k < 5; ++k) o[k] = v[k];
    }
}

// one workgroup, one thread per image at a time: the image's slices in slice order -> partial[b], (SEC) its three expand terms from
// the map statistics in class order; then the means over the batch -> loss.  LDS: block_sum's scratch.
template <bool DSRG>
__global__ __launch_bounds__(SL_FINISH_THREADS) void seg_loss_finish_kernel(const double *__restrict__ chunk, int S,
                                                                             const float *__restrict__ labels,
                                                                             const SlMapStat *__restrict__ stat, int B, int n, int C,
                                                                             double *__restrict__ partial, double *__restrict__ loss) {
    extern __shared__ __attribute__((aligned(16))) char sl_lds[];
    double *scratch = (double *)sl_lds;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // seed (SEC) / seed_bg (DSRG), seed_fg, constrain, loss_1, loss_2, loss_3
    for (int b = threadIdx.x; b < B; b += SL_FINISH_THREADS) {
        double p[SL_P_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < 5; ++k) p[k] += chunk[((size_t)b * S + s) * 5 + k];
        if (!DSRG) {
            const float *lab = labels + (size_t)b * C;
            const SlMapStat *st = stat + (size_t)b * C;
            const double pos = sl_positives(lab, C), neg = (double)(C - 1) - pos;
            for (int c = 1; c < C; ++c) {
                if (lab[c] > 0.f) p[SL_P_L1] += st[c].log_mean / fmax(pos, 1e-5);
                else p[SL_P_L2] += st[c].log_rest / fmax(neg, 1e-5);
            }
            p[SL_P_L3] = st[0].log_mean;
        }
        for (int k = 0; k < SL_P_N; ++k) partial[(size_t)b * SL_P_N + k] = p[k];
        if (DSRG) {
            v[0] += p[SL_P_SEED_BG] / (p[SL_P_CNT_BG] + 1e-8);
            v[1] += p[SL_P_SEED_FG] / (p[SL_P_CNT_FG] + 1e-8);
        } else {
            v[0] += (p[SL_P_SEED_BG] + p[SL_P_SEED_FG]) / fmax(p[SL_P_CNT_BG] + p[SL_P_CNT_FG], 1e-5);
        }
        v[2] += p[SL_P_CONSTRAIN];
        v[3] += p[SL_P_L1];
        v[4] += p[SL_P_L2];
        v[5] += p[SL_P_L3];
    }
    block_sum<6>(v, scratch);
    if (threadIdx.x == 0) {
        const double nb = (double)B;
        const double seed_a = -v[0] / nb, seed_b = -v[1] / nb;
        const double seed = seed_a + seed_b, constrain = v[2] / (nb * (double)n);
        const double l1 = DSRG ? 0.0 : -v[3] / nb, l2 = DSRG ? 0.0 : -v[4] / nb, l3 = DSRG ? 0.0 : -v[5] / nb;
        const double expand = l1 + l2 + l3;
        loss[WSC_SEG_LOSS_SEED] = seed;
        loss[WSC_SEG_LOSS_CONSTRAIN] = constrain;
        loss[WSC_SEG_LOSS_EXPAND] = expand;
        loss[WSC_SEG_LOSS_1] = l1;
        loss[WSC_SEG_LOSS_2] = l2;
        loss[WSC_SEG_LOSS_3] = l3;
        loss[WSC_SEG_LOSS_NORM] = DSRG ? seed + constrain : seed + expand + constrain; // getloss's sum, in its order
        loss[WSC_SEG_LOSS_SEED_BG] = DSRG ? seed_a : 0.0;
        loss[WSC_SEG_LOSS_SEED_FG] = DSRG ? seed_b : 0.0;
    }
}

// grid (ceil(n / SL_GRAD_THREADS), B), one thread per pixel.  g_p and g_z must not overlap the inputs or each other.
template <bool DSRG>
__global__ __launch_bounds__(SL_GRAD_THREADS) void seg_loss_grad_kernel(const float *__restrict__ prob, const float *__restrict__ crf,
                                                                         const float *__restrict__ cues,
                                                                         const float *__restrict__ labels, int n, int C, double m,
                                                                         const float *__restrict__ w_fg, const float *__restrict__ w_bg,
                                                                         double z_fg, double z_bg, const uint16_t *__restrict__ rank,
                                                                         const SlMapStat *__restrict__ stat,
                                                                         const double *__restrict__ partial, float *__restrict__ g_p,
                                                                         float *__restrict__ g_z) {
    const int pix = blockIdx.x * SL_GRAD_THREADS + threadIdx.x, b = blockIdx.y;
    if (pix >= n) return;
    const double inv_b = 1.0 / (double)gridDim.y, inv_bn = inv_b / (double)n, scale = 1.0 + (double)C * m;
    const size_t at = ((size_t)b * n + pix) * C;
    const double *part = partial + (size_t)b * SL_P_N;
    const double den_bg = DSRG ? part[SL_P_CNT_BG] + 1e-8 : fmax(part[SL_P_CNT_BG] + part[SL_P_CNT_FG], 1e-5);
    const double den_fg = DSRG ? part[SL_P_CNT_FG] + 1e-8 : den_bg;
    const float *lab = DSRG ? nullptr : labels + (size_t)b * C;
    double pos = 0.0, neg = 0.0;
    if (!DSRG) {
        pos = sl_positives(lab, C);
        neg = (double)(C - 1) - pos;
    }
    double g[SL_MAX_C]; // registers: the loop below is unrolled, every index a constant
    double dot = 0.0;   // <g, s>, s = p (1 + C m) - m: the plain softmax behind build_sp_softmax
#pragma unroll
    for (int c = 0; c < SL_MAX_C; ++c) {
        g[c] = 0.0;
        if (c < C) {
            const float pf = prob[at + c], cue = cues[at + c];
            const double p = (double)pf, q = exp((double)crf[at + c]);
            double d = 0.0;
            if (cue != 0.f) d -= inv_b * (double)cue / (c ? den_fg : den_bg) / p;
            if (DSRG) {
                const double pe = p + 1e-8, ratio = q / pe;
                d -= inv_bn * q * (ratio / pe) / (ratio + 1e-8);
            } else {
                d -= inv_bn * q / p;
                const SlMapStat s = stat[(size_t)b * C + c];
                const int r = rank[((size_t)b * C + c) * n + pix];
                if (c == 0) {
                    d -= inv_b * ((double)w_bg[r] / z_bg) / s.mean;
                } else if (lab[c] > 0.f) {
                    d -= inv_b / fmax(pos, 1e-5) * ((double)w_fg[r] / z_fg) / s.mean;
                } else if (p == s.vmax) {
                    d += inv_b / fmax(neg, 1e-5) / (1.0 - s.vmax) / (double)s.ties;
                }
            }
            g[c] = d;
            dot += d * (p * scale - m);
        }
    }
#pragma unroll
    for (int c = 0; c < SL_MAX_C; ++c)
        if (c < C) {
            if (g_p) g_p[at + c] = (float)g[c];
            if (g_z) {
                const double s = (double)prob[at + c] * scale - m;
                g_z[at + c] = (float)(s * (g[c] - dot) / scale);
            }
        }
}

template <bool DSRG>
int seg_loss_launch(wsc_ctx *ctx, const float *prob, const float *crf, const float *cues, const float *labels, int B, int n, int C,
                    float min_prob, const float *w_fg_host, float z_fg, const float *w_bg_host, float z_bg, double *loss,
                    float *g_p, float *g_z) {
    // scratch of the call: [rank planes | map statistics | per-image sums | per-slice sums]
    const int total = n * C;
    const int S = std::min(SL_MAX_SLICES, (total + SL_PIXEL_ELEMS - 1) / SL_PIXEL_ELEMS);
    const size_t rank_bytes = DSRG ? 0 : ((size_t)B * C * n * sizeof(uint16_t) + 15) / 16 * 16;
    const size_t stat_bytes = DSRG ? 0 : (size_t)B * C * sizeof(SlMapStat);
    const size_t partial_bytes = (size_t)B * SL_P_N * sizeof(double);
    char *scratch = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, rank_bytes + stat_bytes + partial_bytes + (size_t)B * S * 5 * sizeof(double), (void **)&scratch));
    WscCachedGuard scratch_guard(ctx, scratch);
    uint16_t *rank = (uint16_t *)scratch;
    SlMapStat *stat = (SlMapStat *)(scratch + rank_bytes);
    double *partial = (double *)(scratch + rank_bytes + stat_bytes);
    double *chunk = (double *)(scratch + rank_bytes + stat_bytes + partial_bytes);
    WscStagedTable tab(ctx);
    const float *w_fg = nullptr, *w_bg = nullptr;
    const size_t reduce_lds = (size_t)SL_MAX_WAVES * 6 * sizeof(double);
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * n * C * (12.0 + (g_p ? 4 : 0) + (g_z ? 4 : 0)));
    if (!DSRG) {
        const size_t fg_at = tab.add(w_fg_host, (size_t)n * sizeof(float)), bg_at = tab.add(w_bg_host, (size_t)n * sizeof(float));
        WSC_TRY(tab.upload());
        w_fg = tab.at<const float>(fg_at);
        w_bg = tab.at<const float>(bg_at);
        int P = 1;
        while (P < n) P <<= 1;
        const size_t lds = (size_t)P * sizeof(unsigned long long) + reduce_lds;
        // beyond the 64 KiB a launch gets by default the limit is raised first, and a refusal ends the call
        if (lds > 64 * 1024) WSC_TRY(wsc_set_max_dynamic_lds(ctx, reinterpret_cast<const void *>(seg_loss_rank_kernel), (int)lds));
        hipLaunchKernelGGL(seg_loss_rank_kernel, dim3(C, B), dim3(SL_SORT_THREADS), lds, ctx->stream, prob, n, P, C, w_fg, w_bg,
                           (double)z_fg, (double)z_bg, rank, stat);
        WSC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(seg_loss_pixel_kernel<DSRG>, dim3(S, B), dim3(SL_PIXEL_THREADS), reduce_lds, ctx->stream, prob, crf, cues, n, C,
                       chunk);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(seg_loss_finish_kernel<DSRG>, dim3(1), dim3(SL_FINISH_THREADS), reduce_lds, ctx->stream, (const double *)chunk, S,
                       labels, (const SlMapStat *)stat, B, n, C, partial, loss);
    WSC_HIP(hipGetLastError());
    if (g_p || g_z) {
        hipLaunchKernelGGL(seg_loss_grad_kernel<DSRG>, dim3((n + SL_GRAD_THREADS - 1) / SL_GRAD_THREADS, B), dim3(SL_GRAD_THREADS), 0,
                           ctx->stream, prob, crf, cues, labels, n, C, (double)min_prob, w_fg, w_bg, (double)z_fg, (double)z_bg,
                           (const uint16_t *)rank, (const SlMapStat *)stat, (const double *)partial, g_p, g_z);
        WSC_HIP(hipGetLastError());
    }
    tab.release(); // stream-ordered reuse, as the scratch block
    scratch_guard.free_now();
    return WSC_OK;
}

} // namespace

extern "C" {

int wsc_seg_loss(wsc_ctx *ctx, int method, const float *prob_dev, const float *crf_dev, const float *cues_dev, const float *labels_dev,
                 int B, int H, int W, int C, float min_prob, const float *w_fg_host, float z_fg, const float *w_bg_host, float z_bg,
                 double *loss_dev, float *grad_prob_dev, float *grad_fc8_dev) {
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_seg_loss: ctx is NULL");
    WSC_CHECK(method == WSC_SEG_LOSS_SEC || method == WSC_SEG_LOSS_DSRG, WSC_ERR_INVALID,
              "wsc_seg_loss: method=%d (WSC_SEG_LOSS_SEC or WSC_SEG_LOSS_DSRG)", method);
    WSC_CHECK(prob_dev, WSC_ERR_INVALID, "wsc_seg_loss: prob_dev is NULL");
    WSC_CHECK(crf_dev, WSC_ERR_INVALID, "wsc_seg_loss: crf_dev is NULL");
    WSC_CHECK(cues_dev, WSC_ERR_INVALID, "wsc_seg_loss: cues_dev is NULL");
    WSC_CHECK(loss_dev, WSC_ERR_INVALID, "wsc_seg_loss: loss_dev is NULL");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_seg_loss: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(H >= 1 && W >= 1 && (long long)H * W <= SL_MAX_PIXELS, WSC_ERR_INVALID,
              "wsc_seg_loss: H=%d x W=%d = %lld pixels (both >= 1; a map is sorted in LDS: at most %d pixels)", H, W, (long long)H * W,
              SL_MAX_PIXELS);
    WSC_CHECK(C >= 2 && C <= SL_MAX_C, WSC_ERR_INVALID, "wsc_seg_loss: C=%d (2 <= C <= %d, class 0 is the background)", C, SL_MAX_C);
    WSC_CHECK(min_prob >= 0.f && min_prob < 1.f, WSC_ERR_INVALID, "wsc_seg_loss: min_prob=%g (0 <= min_prob < 1)", (double)min_prob);
    if (method == WSC_SEG_LOSS_SEC) {
        WSC_CHECK(labels_dev, WSC_ERR_INVALID, "wsc_seg_loss: labels_dev is NULL (SEC's expand loss reads the image labels)");
        WSC_CHECK(w_fg_host, WSC_ERR_INVALID, "wsc_seg_loss: w_fg_host is NULL (SEC's rank weights)");
        WSC_CHECK(w_bg_host, WSC_ERR_INVALID, "wsc_seg_loss: w_bg_host is NULL (SEC's rank weights)");
        WSC_CHECK(z_fg > 0.f && z_bg > 0.f, WSC_ERR_INVALID, "wsc_seg_loss: z_fg=%g z_bg=%g (the weight sums are positive)",
                  (double)z_fg, (double)z_bg);
    }
    WSC_CHECK(!grad_prob_dev || grad_prob_dev != grad_fc8_dev, WSC_ERR_INVALID,
              "wsc_seg_loss: grad_prob_dev and grad_fc8_dev are the same buffer");
    WSC_HIP(hipSetDevice(ctx->device));
    if (method == WSC_SEG_LOSS_SEC)
        return seg_loss_launch<false>(ctx, prob_dev, crf_dev, cues_dev, labels_dev, B, H * W, C, min_prob, w_fg_host, z_fg, w_bg_host,
                                      z_bg, loss_dev, grad_prob_dev, grad_fc8_dev);
    return seg_loss_launch<true>(ctx, prob_dev, crf_dev, cues_dev, nullptr, B, H * W, C, min_prob, nullptr, 0.f, nullptr, 0.f, loss_dev,
                                 grad_prob_dev, grad_fc8_dev);
}

} // extern "C"
