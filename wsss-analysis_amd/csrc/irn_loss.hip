// irn_loss.hip -- the IRNet training loss and the gradient it sends into edge_out and dp_out (03b_irn/net/resnet50_irn.py:162-213
// AffinityDisplacementLoss.to_affinity, to_pair_displacement, to_displacement_loss, forward; the pair labels of
// voc12/dataloader.py:115-131 GetAffinityLabelFromIndices; the reductions of step/train_irn.py:114-125).  The formulas:
// include/wsscam.h, wsc_irn_aff_loss.
//
// The reference materialises every (source, direction) pair: an index_select copy per path length, four loss tensors and their
// autograd twins.  Nothing per pair is kept here, because a pair's affinity terms depend on ONE pixel, the first pixel of its
// path that holds the maximum logit m: pos(m) and neg(m) are functions of that pixel's logit alone.  So
//     sum over bg pairs of pos  =  sum over pixels p of  cnt_bg(p) pos(e_p),        d total / d e_p  =  sum_class cnt_class(p) coeff_class pos'(e_p)
// with cnt_class(p) the NUMBER of pairs of that class whose path maximum sits at p -- an integer.  Likewise d|v|/dv is -1, 0
// or 1, so the displacement gradient of a pixel is (an integer sum of signs) x (one weight per class).  The pair pass therefore
// only counts, with integer atomics, which are exact whatever their order; every transcendental runs once per pixel, not once
// per pair (2134 path pixels per source at radius 10), and the only per-pair floating-point sums are the two displacement losses.
//
//   irn_pair_kernel    a workgroup owns a tile of 8 x 32 sources (a 32-lane group reads one row: bank-conflict free) and stages
//                      the logits, both dp channels and the labels of the tile plus halo (rf rows below, rf columns either side)
//                      in LDS next to seven integer planes.  A thread owns one source and walks the directions: valid pairs
//                      walk their path for the first maximum and count it at that pixel (LDS integer atomic); bg / fg pairs add
//                      |pd - target| to the thread's double sum and the signs to the source (registers) and the destination.
//                      The planes are flushed to HBM with integer atomics (halos overlap); the five sums of the block go to
//                      partial[block] through block_sum.
//   irn_reduce_kernel  one workgroup: the per-block partials in block order (a thread adds its strided share in index order,
//                      block_sum adds the threads).  Its second use also forms the ten loss slots.
//   irn_pixel_kernel   one thread per pixel: sigmoid, the two logs and their derivatives of the pixel's logit, the three
//                      count-weighted affinity sums of the block, and both gradients (every element written, plain +0.0 where
//                      no pair reaches).
// Inputs are float32; every sigmoid, log, product and sum is double and every output is rounded once.  No floating-point atomic.
#include <limits.h>

#include <algorithm>
#include <cstdlib>

#include "common.h"

namespace {

constexpr int IL_TX = 32, IL_TY = 8, IL_THREADS = IL_TX * IL_TY;
constexpr int IL_MAX_RF = 16; // tile + halo at the limit: (8 + 16) x (32 + 32) cells of 41 bytes = 63 KB of LDS
constexpr int IL_WAVES = IL_THREADS / 64;
// integer planes [B][IL_PLANES][h][w]: pairs whose path maximum sits at the pixel, per class; sums of d|v|/dv per class and channel
enum { IL_CNT_BG = 0, IL_CNT_FG, IL_CNT_NEG, IL_SGN_FG0, IL_SGN_FG1, IL_SGN_BG0, IL_SGN_BG1, IL_PLANES };
// sums of the call, double [IL_SUMS]: the pair pass's five, then the pixel pass's three
enum { IL_DP_FG = 0, IL_DP_BG, IL_N_BG, IL_N_FG, IL_N_NEG, IL_PAIR_SUMS, IL_POS_BG = IL_PAIR_SUMS, IL_POS_FG, IL_NEG, IL_SUMS };
constexpr int IL_PIXEL_SUMS = IL_SUMS - IL_PAIR_SUMS;
constexpr int IL_CELL_BYTES = 3 * sizeof(float) + IL_PLANES * sizeof(int) + 1;

struct IlShape {
    int h, w, rf, D, valid_below;
    int ntx;    // tiles across
    int TW, TH; // the staged tile: IL_TX + 2 rf columns, IL_TY + rf rows
};

__device__ __forceinline__ int il_sign(double v) { return (v > 0.0) - (v < 0.0); }

// grid (tiles, B).  Dynamic LDS: TW * TH cells [logit | dp_0 | dp_1 | IL_PLANES ints | label].  path_off: a path pixel's offset
// in the staged tile, dy * TW + dx.
__global__ __launch_bounds__(IL_THREADS) void irn_pair_kernel(const float *__restrict__ edge, const float *__restrict__ dp,
                                                               const uint8_t *__restrict__ label, IlShape s,
                                                               const int32_t *__restrict__ dirs, const int32_t *__restrict__ path_start,
                                                               const int32_t *__restrict__ path_off, int *__restrict__ planes,
                                                               double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char il_lds[];
    __shared__ double scratch[IL_WAVES * IL_PAIR_SUMS];
    const int n = s.TW * s.TH, hw = s.h * s.w, tid = threadIdx.x;
    float *le = (float *)il_lds, *ld0 = le + n, *ld1 = ld0 + n;
    int *lc = (int *)(ld1 + n);
    uint8_t *ll = (uint8_t *)(lc + IL_PLANES * n);
    const int b = blockIdx.y, ty = (int)blockIdx.x / s.ntx, tx = (int)blockIdx.x - ty * s.ntx;
    const int y0 = ty * IL_TY, x0 = tx * IL_TX; // image position of cell (0, 0); the source of lane (ly, lx) is cell (ly, lx + rf)
    const float *e_img = edge + (size_t)b * hw, *d_img = dp + (size_t)b * 2 * hw;
    const uint8_t *l_img = label + (size_t)b * hw;
    for (int i = tid; i < n; i += IL_THREADS) {
        const int r = i / s.TW, yy = y0 + r, xx = x0 + (i - r * s.TW);
        const bool in = yy < s.h && xx < s.w;
        const int at = yy * s.w + xx;
        le[i] = in ? e_img[at] : 0.f;
        ld0[i] = in ? d_img[at] : 0.f;
        ld1[i] = in ? d_img[hw + at] : 0.f;
        ll[i] = in ? l_img[at] : (uint8_t)255;
    }
    for (int i = tid; i < IL_PLANES * n; i += IL_THREADS) lc[i] = 0;
    __syncthreads();
    const int ly = tid / IL_TX, lx = tid - ly * IL_TX;
    const int me = ly * s.TW + lx + s.rf;
    double v[IL_PAIR_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // a source: y < h - rf, rf <= x < w - rf, so every destination and path pixel is on the image and inside the staged tile
    if (y0 + ly < s.h - s.rf && x0 + lx + s.rf < s.w - s.rf && (int)ll[me] < s.valid_below) {
        const int Ls = ll[me];
        const double a0 = (double)ld0[me], a1 = (double)ld1[me];
        int n_bg = 0, n_fg = 0, n_neg = 0, sg[4] = {0, 0, 0, 0}; // IL_SGN_FG0 .. IL_SGN_BG1 of this source
        for (int d = 0; d < s.D; ++d) {
            const int dy = dirs[2 * d], dx = dirs[2 * d + 1]; // (uniform)
            const int t = me + dy * s.TW + dx;
            const int Lt = ll[t];
            if (Lt >= s.valid_below) continue;
            // the first pixel in stored path order that holds the maximum logit
            int c = path_start[d];
            const int c1 = path_start[d + 1];
            int arg = me + path_off[c];
            float m = le[arg];
            for (++c; c < c1; ++c) {
                const int o = me + path_off[c];
                const float val = le[o];
                if (val > m || val != val) { // (a NaN logit is the path's maximum, as torch's max makes it: the pair's term is NaN)
                    m = val;
                    arg = o;
                }
            }
            if (Ls != Lt) {
                ++n_neg;
                atomicAdd(&lc[IL_CNT_NEG * n + arg], 1);
                continue;
            }
            const int fg = Ls > 0;
            atomicAdd(&lc[(fg ? IL_CNT_FG : IL_CNT_BG) * n + arg], 1);
            const double pd0 = a0 - (double)ld0[t], pd1 = a1 - (double)ld1[t];
            const double v0 = fg ? pd0 - (double)dy : pd0, v1 = fg ? pd1 - (double)dx : pd1;
            v[fg ? IL_DP_FG : IL_DP_BG] += fabs(v0) + fabs(v1);
            n_fg += fg;
            n_bg += 1 - fg;
            const int s0 = il_sign(v0), s1 = il_sign(v1), k = fg ? 0 : 2;
            sg[k] += s0;
            sg[k + 1] += s1;
            if (s0) atomicAdd(&lc[(IL_SGN_FG0 + k) * n + t], -s0); // pd = dp(s) - dp(t): the destination takes the opposite sign
            if (s1) atomicAdd(&lc[(IL_SGN_FG0 + k + 1) * n + t], -s1);
        }
        for (int k = 0; k < 4; ++k)
            if (sg[k]) atomicAdd(&lc[(IL_SGN_FG0 + k) * n + me], sg[k]);
        v[IL_N_BG] = (double)n_bg;
        v[IL_N_FG] = (double)n_fg;
        v[IL_N_NEG] = (double)n_neg;
    }
    __syncthreads();
    int *out = planes + (size_t)b * IL_PLANES * hw;
    for (int i = tid; i < IL_PLANES * n; i += IL_THREADS) {
        const int val = lc[i];
        if (!val) continue;
        const int k = i / n, cell = i - k * n, r = cell / s.TW, yy = y0 + r, xx = x0 + (cell - r * s.TW);
        if (yy < s.h && xx < s.w) atomicAdd(&out[(size_t)k * hw + yy * s.w + xx], val); // (integers: exact in any order)
    }
    block_sum<IL_PAIR_SUMS>(v, scratch);
    if (tid == 0) {
        double *o = partial + ((size_t)b * gridDim.x + blockIdx.x) * IL_PAIR_SUMS;
        for (int k = 0; k < IL_PAIR_SUMS; ++k) o[k] = v[k];
    }
}

// sigmoid(-e) and sigmoid(e) without cancellation or overflow: exp of a non-positive number only
__device__ __forceinline__ void il_sigmoid_pair(double e, double *aff, double *rest) {
    const double ex = exp(-fabs(e)), big = 1.0 / (1.0 + ex), small = ex * big;
    *aff = e >= 0.0 ? small : big; // 1 - sigmoid(e)
    *rest = e >= 0.0 ? big : small;
}

// grid (ceil(h w / IL_THREADS), B).  sums: the pair pass's five.  partial [B][gridDim.x][IL_PIXEL_SUMS].
__global__ __launch_bounds__(IL_THREADS) void irn_pixel_kernel(const float *__restrict__ edge, const int *__restrict__ planes, int hw,
                                                                const double *__restrict__ sums, double *__restrict__ partial,
                                                                float *__restrict__ g_edge, float *__restrict__ g_dp) {
    __shared__ double scratch[IL_WAVES * IL_PIXEL_SUMS];
    const int b = blockIdx.y, i = blockIdx.x * IL_THREADS + threadIdx.x;
    double v[IL_PIXEL_SUMS] = {0.0, 0.0, 0.0};
    if (i < hw) {
        const int *pl = planes + (size_t)b * IL_PLANES * hw + i;
        const int c_bg = pl[IL_CNT_BG * (size_t)hw], c_fg = pl[IL_CNT_FG * (size_t)hw], c_neg = pl[IL_CNT_NEG * (size_t)hw];
        const double n_bg = sums[IL_N_BG], n_fg = sums[IL_N_FG], n_neg = sums[IL_N_NEG];
        double ge = 0.0;
        if (c_bg | c_fg | c_neg) {
            double aff, rest;
            il_sigmoid_pair((double)edge[(size_t)b * hw + i], &aff, &rest);
            const double p_arg = aff + 1e-5, n_arg = 1.0 + 1e-5 - aff;
            const double pos = -log(p_arg), neg = -log(n_arg);
            const double d_aff = aff * rest; // -d aff / d e
            const double d_pos = d_aff / p_arg, d_neg = -d_aff / n_arg;
            v[0] = (double)c_bg * pos;
            v[1] = (double)c_fg * pos;
            v[2] = (double)c_neg * neg;
            // total = (pos_bg / 2 + pos_fg / 2 + neg) / 2 + ...
            if (c_bg) ge += (double)c_bg * d_pos * (0.25 / (n_bg + 1e-5));
            if (c_fg) ge += (double)c_fg * d_pos * (0.25 / (n_fg + 1e-5));
            if (c_neg) ge += (double)c_neg * d_neg * (0.5 / (n_neg + 1e-5));
        }
        if (g_edge) g_edge[(size_t)b * hw + i] = (float)ge;
        if (g_dp) {
            const double w_fg = 0.5 / (2.0 * n_fg + 1e-5), w_bg = 0.5 / (2.0 * n_bg + 1e-5); // total = ... + (dp_fg + dp_bg) / 2
            for (int c = 0; c < 2; ++c) {
                const int s_fg = pl[(IL_SGN_FG0 + c) * (size_t)hw], s_bg = pl[(IL_SGN_BG0 + c) * (size_t)hw];
                double g = 0.0;
                if (s_fg) g += (double)s_fg * w_fg;
                if (s_bg) g += (double)s_bg * w_bg;
                g_dp[((size_t)b * 2 + c) * hw + i] = (float)g;
            }
        }
    }
    block_sum<IL_PIXEL_SUMS>(v, scratch);
    if (threadIdx.x == 0) {
        double *o = partial + ((size_t)b * gridDim.x + blockIdx.x) * IL_PIXEL_SUMS;
        for (int k = 0; k < IL_PIXEL_SUMS; ++k) o[k] = v[k];
    }
}

// one workgroup: out[k] = sum over the n blocks of partial[block][k], in block order.  loss != nullptr: `out` completes `sums`
// (the pixel pass's three after the pair pass's five) and the ten slots are formed.
template <int NV>
__global__ __launch_bounds__(IL_THREADS) void irn_reduce_kernel(const double *__restrict__ partial, long long n, double *__restrict__ out,
                                                                 const double *__restrict__ sums, double *__restrict__ loss) {
    __shared__ double scratch[IL_WAVES * NV];
    double v[NV];
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (long long i = threadIdx.x; i < n; i += IL_THREADS)
        for (int k = 0; k < NV; ++k) v[k] += partial[i * NV + k];
    block_sum<NV>(v, scratch);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < NV; ++k) out[k] = v[k];
    if (!loss) return;
    const double n_bg = sums[IL_N_BG], n_fg = sums[IL_N_FG], n_neg = sums[IL_N_NEG];
    const double pos_bg = v[IL_POS_BG - IL_PAIR_SUMS] / (n_bg + 1e-5), pos_fg = v[IL_POS_FG - IL_PAIR_SUMS] / (n_fg + 1e-5);
    const double pos = pos_bg / 2.0 + pos_fg / 2.0, neg = v[IL_NEG - IL_PAIR_SUMS] / (n_neg + 1e-5);
    const double dp_fg = sums[IL_DP_FG] / (2.0 * n_fg + 1e-5), dp_bg = sums[IL_DP_BG] / (2.0 * n_bg + 1e-5);
    loss[WSC_IRN_LOSS_POS_BG] = pos_bg;
    loss[WSC_IRN_LOSS_POS_FG] = pos_fg;
    loss[WSC_IRN_LOSS_POS] = pos;
    loss[WSC_IRN_LOSS_NEG] = neg;
    loss[WSC_IRN_LOSS_DP_FG] = dp_fg;
    loss[WSC_IRN_LOSS_DP_BG] = dp_bg;
    loss[WSC_IRN_LOSS_TOTAL] = (pos + neg) / 2.0 + (dp_fg + dp_bg) / 2.0;
    loss[WSC_IRN_LOSS_N_BG] = n_bg;
    loss[WSC_IRN_LOSS_N_FG] = n_fg;
    loss[WSC_IRN_LOSS_N_NEG] = n_neg;
}

bool il_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

} // namespace

extern "C" int wsc_irn_aff_loss(wsc_ctx *ctx, const float *edge_dev, const float *dp_dev, const uint8_t *label_dev, int B, int h, int w,
                                const int32_t *dirs_host, const int32_t *path_start_host, const int32_t *path_yx_host, int D,
                                int radius_floor, int valid_below, double *loss_dev, float *grad_edge_dev, float *grad_dp_dev) {
    const int rf = radius_floor;
    WSC_CHECK(ctx, WSC_ERR_INVALID, "wsc_irn_aff_loss: ctx is NULL");
    WSC_CHECK(edge_dev, WSC_ERR_INVALID, "wsc_irn_aff_loss: edge_dev is NULL");
    WSC_CHECK(dp_dev, WSC_ERR_INVALID, "wsc_irn_aff_loss: dp_dev is NULL");
    WSC_CHECK(label_dev, WSC_ERR_INVALID, "wsc_irn_aff_loss: label_dev is NULL");
    WSC_CHECK(loss_dev, WSC_ERR_INVALID, "wsc_irn_aff_loss: loss_dev is NULL");
    WSC_CHECK(dirs_host, WSC_ERR_INVALID, "wsc_irn_aff_loss: dirs_host is NULL");
    WSC_CHECK(path_start_host, WSC_ERR_INVALID, "wsc_irn_aff_loss: path_start_host is NULL");
    WSC_CHECK(path_yx_host, WSC_ERR_INVALID, "wsc_irn_aff_loss: path_yx_host is NULL");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_irn_aff_loss: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(rf >= 0 && rf <= IL_MAX_RF, WSC_ERR_INVALID,
              "wsc_irn_aff_loss: radius_floor=%d (0 <= radius_floor <= %d: a tile and its halo live in LDS)", rf, IL_MAX_RF);
    WSC_CHECK(h > rf && w > 2 * rf, WSC_ERR_INVALID, "wsc_irn_aff_loss: h=%d w=%d leave no source (h > radius_floor = %d, w > %d)", h,
              w, rf, 2 * rf);
    WSC_CHECK((long long)h * w <= INT_MAX / 8, WSC_ERR_INVALID, "wsc_irn_aff_loss: h=%d x w=%d = %lld pixels (at most %d)", h, w,
              (long long)h * w, INT_MAX / 8);
    WSC_CHECK(D >= 1, WSC_ERR_INVALID, "wsc_irn_aff_loss: D=%d (at least one direction)", D);
    WSC_CHECK(valid_below >= 1 && valid_below <= 255, WSC_ERR_INVALID, "wsc_irn_aff_loss: valid_below=%d (1 .. 255; 255 is the ignore label)",
              valid_below);
    WSC_CHECK(path_start_host[0] == 0, WSC_ERR_INVALID, "wsc_irn_aff_loss: path_start_host[0]=%d (the table starts at 0)", path_start_host[0]);
    for (int d = 0; d < D; ++d) {
        WSC_CHECK(path_start_host[d] < path_start_host[d + 1], WSC_ERR_INVALID,
                  "wsc_irn_aff_loss: path_start_host: the path of direction %d is empty or the table decreases", d);
        WSC_CHECK(dirs_host[2 * d] >= 0 && dirs_host[2 * d] <= rf && std::abs(dirs_host[2 * d + 1]) <= rf, WSC_ERR_INVALID,
                  "wsc_irn_aff_loss: dirs_host: direction %d = (%d, %d) leaves [0, %d] x [-%d, %d]", d, dirs_host[2 * d],
                  dirs_host[2 * d + 1], rf, rf, rf);
    }
    const int n_path = path_start_host[D];
    for (int c = 0; c < n_path; ++c)
        WSC_CHECK(path_yx_host[2 * c] >= 0 && path_yx_host[2 * c] <= rf && std::abs(path_yx_host[2 * c + 1]) <= rf, WSC_ERR_INVALID,
                  "wsc_irn_aff_loss: path_yx_host: path pixel %d = (%d, %d) leaves [0, %d] x [-%d, %d]", c, path_yx_host[2 * c],
                  path_yx_host[2 * c + 1], rf, rf, rf);
    const size_t hw = (size_t)h * w, edge_bytes = (size_t)B * hw * sizeof(float);
    const struct { const void *p; size_t bytes; const char *name; } inputs[4] = {{edge_dev, edge_bytes, "edge_dev"},
                                                                                   {dp_dev, 2 * edge_bytes, "dp_dev"},
                                                                                   {label_dev, (size_t)B * hw, "label_dev"},
                                                                                   {loss_dev, WSC_IRN_LOSS_N * sizeof(double), "loss_dev"}};
    for (const auto &in : inputs) {
        WSC_CHECK(!grad_edge_dev || !il_overlap(grad_edge_dev, edge_bytes, in.p, in.bytes), WSC_ERR_INVALID,
                  "wsc_irn_aff_loss: grad_edge_dev overlaps %s", in.name);
        WSC_CHECK(!grad_dp_dev || !il_overlap(grad_dp_dev, 2 * edge_bytes, in.p, in.bytes), WSC_ERR_INVALID,
                  "wsc_irn_aff_loss: grad_dp_dev overlaps %s", in.name);
    }
    WSC_CHECK(!grad_edge_dev || !grad_dp_dev || !il_overlap(grad_edge_dev, edge_bytes, grad_dp_dev, 2 * edge_bytes), WSC_ERR_INVALID,
              "wsc_irn_aff_loss: grad_edge_dev overlaps grad_dp_dev");
    WSC_HIP(hipSetDevice(ctx->device));

    IlShape s;
    s.h = h; s.w = w; s.rf = rf; s.D = D; s.valid_below = valid_below;
    s.ntx = (w - 2 * rf + IL_TX - 1) / IL_TX;
    s.TW = IL_TX + 2 * rf;
    s.TH = IL_TY + rf;
    const int nty = (h - rf + IL_TY - 1) / IL_TY, tiles = s.ntx * nty, pixel_blocks = (int)((hw + IL_THREADS - 1) / IL_THREADS);
    const size_t lds = (size_t)s.TW * s.TH * IL_CELL_BYTES;
    std::vector<int32_t> path_off(n_path);
    for (int c = 0; c < n_path; ++c) path_off[c] = path_yx_host[2 * c] * s.TW + path_yx_host[2 * c + 1];
    WscStagedTable tab(ctx);
    const size_t dirs_at = tab.add(dirs_host, (size_t)2 * D * sizeof(int32_t));
    const size_t start_at = tab.add(path_start_host, (size_t)(D + 1) * sizeof(int32_t)), off_at = tab.add(path_off);
    WSC_TRY(tab.upload());
    // scratch of the call: [integer planes | sums | pair-pass partials | pixel-pass partials]
    const size_t plane_bytes = ((size_t)B * IL_PLANES * hw * sizeof(int) + 15) / 16 * 16;
    const size_t pair_part = (size_t)B * tiles * IL_PAIR_SUMS, pixel_part = (size_t)B * pixel_blocks * IL_PIXEL_SUMS;
    char *scratch = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, plane_bytes + (IL_SUMS + pair_part + pixel_part) * sizeof(double), (void **)&scratch));
    WscCachedGuard scratch_guard(ctx, scratch);
    int *planes = (int *)scratch;
    double *sums = (double *)(scratch + plane_bytes), *partial_pair = sums + IL_SUMS, *partial_pixel = partial_pair + pair_part;
    // bytes: the staged tiles (halo included), the planes zeroed, added to and read, the gradients
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * tiles * s.TW * s.TH * 13.0 + 3.0 * (double)plane_bytes +
                                                   (double)B * hw * 4.0 * (1 + (grad_edge_dev ? 1 : 0) + (grad_dp_dev ? 2 : 0)));
    WSC_HIP(hipMemsetAsync(planes, 0, plane_bytes, ctx->stream));
    hipLaunchKernelGGL(irn_pair_kernel, dim3(tiles, B), dim3(IL_THREADS), lds, ctx->stream, edge_dev, dp_dev, label_dev, s,
                       tab.at<const int32_t>(dirs_at), tab.at<const int32_t>(start_at), tab.at<const int32_t>(off_at), planes,
                       partial_pair);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(irn_reduce_kernel<IL_PAIR_SUMS>, dim3(1), dim3(IL_THREADS), 0, ctx->stream, (const double *)partial_pair,
                       (long long)B * tiles, sums, (const double *)nullptr, (double *)nullptr);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(irn_pixel_kernel, dim3(pixel_blocks, B), dim3(IL_THREADS), 0, ctx->stream, edge_dev, (const int *)planes, (int)hw,
                       (const double *)sums, partial_pixel, grad_edge_dev, grad_dp_dev);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(irn_reduce_kernel<IL_PIXEL_SUMS>, dim3(1), dim3(IL_THREADS), 0, ctx->stream, (const double *)partial_pixel,
                       (long long)B * pixel_blocks, sums + IL_PAIR_SUMS, (const double *)sums, loss_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse, as the scratch block
    scratch_guard.free_now();
    return WSC_OK;
}
