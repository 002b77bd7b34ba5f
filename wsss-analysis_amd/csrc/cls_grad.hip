// cls_grad.hip -- BatchNorm in training mode, forward and backward: the new kernels of the 01_train backward pass through the plain
// stacks (VGG16 / M7: conv -> ReLU -> BatchNorm(eps = 1e-3), common_cnn.py:128-141).  The contract: include/wsscam.h
// (wsc_batch_norm_train_nhwc, wsc_batch_norm_grad_nhwc).  The pass that chains them: net.hip (wsc_net_forward_cls_train,
// wsc_net_backward_cls); the pool gradients: pool.hip; the GEMMs: seg_grad.hip.
//
// Both directions are bandwidth-bound column reductions over a [M][C] fp32 matrix with C innermost, followed by an elementwise
// pass.  One reduction skeleton serves both:
//   grid (row blocks, ceil(C / 64)); a block owns `rows_per` rows of a 64-channel slab; thread (lane r = tid / 16, group g = tid % 16)
//   reads 16 bytes -- channels 4 g .. 4 g + 3 of the slab -- of rows r, r + 16, ... and keeps two double sums per channel;
//   the 16 lanes of a channel are added in lane order through LDS; the block's partial goes to partials[slab][block][channel];
//   the last block of a slab to arrive (an integer ticket, agent-scope release / acquire: the pattern of channel_mean_kernel) adds
//   the partials in block order and finishes the slab's channels.
// No floating-point atomic, one fixed order: two calls give the same bits (on one device: the block count follows the CU count).
//   forward   the sums are of d = a - p and d d with the pivot p = a[0][c], formed in double (d is exact): mean = p + S / M,
//             var = Q / M - (S / M)^2 without the cancellation of sum a^2 / M - mean^2 (a channel of mean 1e3 and std 1e-2 keeps its
//             variance to double precision, a constant channel has var = 0 exactly)
//   backward  the sums are of dy and dy xh, xh = (a - mean) rstd in fp32 from the taped float statistics
// The file is compiled with the default contraction; the fused operations of the elementwise passes are spelled, and a - mean
// followed by a product cannot fuse, so the 16-byte form is the only form and every element takes the same roundings.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int BN_BLOCK = 256;      // threads
constexpr int BN_SLAB = 64;        // channels of a block
constexpr int BN_LANES = BN_BLOCK / (BN_SLAB / 4); // rows in flight
constexpr int BN_MAX_BLOCKS = 512; // row blocks = partials of a channel
constexpr int BN_MAX_C = 1024;

struct BnSumArgs {
    const float *a;        // [M][C]
    const float *dy;       // [M][C] (backward)
    const float2 *stats;   // [C] {mean, rstd}: written by the forward finish, read by the backward sums
    long long M, rows_per;
    int C;
    double2 *partials;     // [slabs][gridDim.x][BN_SLAB]
    unsigned *tickets;     // [slabs], zero at launch
    // the forward finish
    float eps, keep;
    int unbiased;
    float *run;            // [2][C] or null
    float2 *stats_out;
    // the backward finish
    float *dgamma, *dbeta; // [C]
    float2 *coef;          // [C] {float(sum dy / M), float(sum dy xh / M)}: what the elementwise pass subtracts
};

template <bool GRAD>
__global__ __launch_bounds__(BN_BLOCK) void bn_sums_kernel(BnSumArgs a) {
    __shared__ double2 red[BN_LANES][BN_SLAB];
    __shared__ int s_last;
    const int tid = threadIdx.x, g = tid & (BN_SLAB / 4 - 1), lane = tid / (BN_SLAB / 4), slab = blockIdx.y;
    const int c0 = slab * BN_SLAB + 4 * g;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    if (c0 < a.C) { // (C is a multiple of 4: a group is inside or outside as a whole)
        const long long r0 = (long long)blockIdx.x * a.rows_per, r1 = min(r0 + a.rows_per, a.M);
        f32x4_t p; // forward: the pivot; backward: the mean
        f32x4_t rs = {0.f, 0.f, 0.f, 0.f};
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 st = a.stats[c0 + j];
                p[j] = st.x;
                rs[j] = st.y;
            }
        } else {
            p = *reinterpret_cast<const f32x4_t *>(a.a + c0);
        }
        for (long long r = r0 + lane; r < r1; r += BN_LANES) {
            const f32x4_t v = *reinterpret_cast<const f32x4_t *>(a.a + r * a.C + c0);
            if (GRAD) {
                const f32x4_t d = *reinterpret_cast<const f32x4_t *>(a.dy + r * a.C + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xh = (v[j] - p[j]) * rs[j];
                    s[j] += (double)d[j];
                    q[j] += (double)d[j] * (double)xh;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = (double)v[j] - (double)p[j];
                    s[j] += d;
                    q[j] += d * d;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[lane][4 * g + j] = make_double2(s[j], q[j]);
    __syncthreads();
    const int c = slab * BN_SLAB + tid; // (tid < BN_SLAB: wave 0 owns the slab's channels from here on)
    double2 *mine = a.partials + ((long long)slab * gridDim.x) * BN_SLAB;
    if (tid < BN_SLAB) {
        double2 t = make_double2(0.0, 0.0);
        for (int l = 0; l < BN_LANES; ++l) {
            t.x += red[l][tid].x;
            t.y += red[l][tid].y;
        }
        mine[(long long)blockIdx.x * BN_SLAB + tid] = t;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(a.tickets + slab, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == gridDim.x - 1;
        if (s_last) { // every block's partial of this slab is out
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last || tid >= BN_SLAB || c >= a.C) return;
    double S = 0.0, Q = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) { // block order
        const double2 t = mine[(long long)b * BN_SLAB + tid];
        S += t.x;
        Q += t.y;
    }
    const double Md = (double)a.M;
    if (GRAD) {
        a.dbeta[c] = (float)S;
        a.dgamma[c] = (float)Q;
        a.coef[c] = make_float2((float)(S / Md), (float)(Q / Md));
    } else {
        const double ms = S / Md;
        const double mean = (double)a.a[c] + ms;
        double var = Q / Md - ms * ms;
        if (var < 0.0) var = 0.0; // (a NaN stays one)
        a.stats_out[c] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)a.eps)));
        if (a.run) {
            const double keep = (double)a.keep, vb = a.unbiased ? var * (Md / (Md - 1.0)) : var;
            a.run[c] = (float)(keep * (double)a.run[c] + (1.0 - keep) * mean);
            a.run[a.C + c] = (float)(keep * (double)a.run[a.C + c] + (1.0 - keep) * vb);
        }
    }
}

// y = (a - mean) rstd gamma + beta, the expression of gn_affine (irn_kernels.hip): what the GroupNorm heads' store computes, so that
// the activation planes launch_group_norm_apply writes from the same statistics hold this value's split
__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ a, const float2 *__restrict__ stats,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta, long long M, int C,
                                                       float *__restrict__ y) {
    const int C4 = C >> 2;
    const long long total = M * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % C4) * 4;
        f32x4_t v = *reinterpret_cast<const f32x4_t *>(a + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 st = stats[c0 + j];
            v[j] = __builtin_fmaf((v[j] - st.x) * st.y, gamma[c0 + j], beta[c0 + j]);
        }
        *reinterpret_cast<f32x4_t *>(y + i * 4) = v;
    }
}

// da = (gamma rstd) ((dy - mb) - xh mg), {mb, mg} = coef: every product and difference one fp32 rounding, xh mg fused into the
// second difference
__global__ __launch_bounds__(256) void bn_grad_apply_kernel(const float *__restrict__ a, const float *__restrict__ dy,
                                                            const float2 *__restrict__ stats, const float2 *__restrict__ coef,
                                                            const float *__restrict__ gamma, long long M, int C, float *__restrict__ da) {
    const int C4 = C >> 2;
    const long long total = M * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % C4) * 4;
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(a + i * 4), d = *reinterpret_cast<const f32x4_t *>(dy + i * 4);
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 st = stats[c0 + j], cf = coef[c0 + j];
            const float xh = (v[j] - st.x) * st.y;
            o[j] = (gamma[c0 + j] * st.y) * __builtin_fmaf(-xh, cf.y, d[j] - cf.x);
        }
        *reinterpret_cast<f32x4_t *>(da + i * 4) = o;
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int bn_shape_check(const char *who, long long M, int C) {
    WSC_CHECK(M >= 1 && M < (1ll << 31) && C >= 4 && C % 4 == 0 && C <= BN_MAX_C, WSC_ERR_INVALID,
              "%s: %lld x %d (1 <= M < 2^31, C a multiple of 4 up to %d)", who, M, C, BN_MAX_C);
    return WSC_OK;
}

// the grid of the sums and one cached block of scratch for it: [tickets | coef (backward) | partials]
struct BnScratch {
    int slabs, blocks;
    long long rows_per;
    size_t coef_at, partials_at, bytes;
    BnScratch(const wsc_ctx *ctx, long long M, int C) {
        slabs = (C + BN_SLAB - 1) / BN_SLAB;
        const long long cap = std::max(1, std::min(BN_MAX_BLOCKS, 4 * (ctx->num_cus > 0 ? ctx->num_cus : 256) / slabs));
        const long long want = std::min(std::max((M + 4 * BN_LANES - 1) / (4 * BN_LANES), 1ll), cap);
        rows_per = (M + want - 1) / want;
        blocks = (int)((M + rows_per - 1) / rows_per); // (no block without rows)
        coef_at = 256;
        partials_at = coef_at + ((size_t)C * sizeof(float2) + 255) / 256 * 256;
        bytes = partials_at + sizeof(double2) * (size_t)slabs * blocks * BN_SLAB;
    }
};

} // namespace

int launch_batch_norm_train(wsc_ctx *ctx, const float *a, long long M, int C, const float *gamma, const float *beta, float eps, float keep,
                            int unbiased, float *run, float *stats, float *y) {
    WSC_TRY(bn_shape_check("BatchNorm (training)", M, C));
    WSC_CHECK(aligned16(a) && (!y || aligned16(y)) && ((uintptr_t)stats & 7u) == 0, WSC_ERR_INVALID,
              "BatchNorm (training): a / y must be 16-byte aligned, stats 8-byte aligned");
    WSC_CHECK(eps >= 0.f && eps < INFINITY, WSC_ERR_INVALID, "BatchNorm (training): eps = %g", (double)eps);
    WSC_CHECK(!run || (keep >= 0.f && keep <= 1.f), WSC_ERR_INVALID, "BatchNorm (training): keep = %g (the weight of the old running value, 0 .. 1)",
              (double)keep);
    WSC_CHECK(!(unbiased && M == 1), WSC_ERR_INVALID, "BatchNorm (training): the unbiased running variance needs M > 1");
    const BnScratch sc(ctx, M, C);
    void *blk = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, sc.bytes, &blk));
    WscCachedGuard guard(ctx, blk);
    BnSumArgs s = {};
    s.a = a; s.M = M; s.rows_per = sc.rows_per; s.C = C;
    s.tickets = (unsigned *)blk;
    s.partials = (double2 *)((char *)blk + sc.partials_at);
    s.eps = eps; s.keep = keep; s.unbiased = unbiased; s.run = run; s.stats_out = (float2 *)stats;
    WSC_HIP(hipMemsetAsync(s.tickets, 0, 256, ctx->stream)); // (the tickets start at zero whatever the block held)
    {
        WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 4.0 * M * C);
        hipLaunchKernelGGL(bn_sums_kernel<false>, dim3(sc.blocks, sc.slabs), dim3(BN_BLOCK), 0, ctx->stream, s);
        WSC_HIP(hipGetLastError());
    }
    guard.free_now();
    if (!y) return WSC_OK;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 8.0 * M * C);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(wsc_grid_for(M * (C / 4))), dim3(256), 0, ctx->stream, a, (const float2 *)stats, gamma, beta, M, C, y);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_batch_norm_grad(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *dy, long long M, int C,
                           float *da, float *dgamma, float *dbeta) {
    WSC_TRY(bn_shape_check("BatchNorm gradient", M, C));
    WSC_CHECK(aligned16(a) && aligned16(dy) && aligned16(da) && ((uintptr_t)stats & 7u) == 0, WSC_ERR_INVALID,
              "BatchNorm gradient: a / dy / da must be 16-byte aligned, stats 8-byte aligned");
    const BnScratch sc(ctx, M, C);
    void *blk = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, sc.bytes, &blk));
    WscCachedGuard guard(ctx, blk);
    BnSumArgs s = {};
    s.a = a; s.dy = dy; s.stats = (const float2 *)stats; s.M = M; s.rows_per = sc.rows_per; s.C = C;
    s.tickets = (unsigned *)blk;
    s.coef = (float2 *)((char *)blk + sc.coef_at);
    s.partials = (double2 *)((char *)blk + sc.partials_at);
    s.dgamma = dgamma; s.dbeta = dbeta;
    WSC_HIP(hipMemsetAsync(s.tickets, 0, 256, ctx->stream));
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 20.0 * M * C);
    hipLaunchKernelGGL(bn_sums_kernel<true>, dim3(sc.blocks, sc.slabs), dim3(BN_BLOCK), 0, ctx->stream, s);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_grad_apply_kernel, dim3(wsc_grid_for(M * (C / 4))), dim3(256), 0, ctx->stream, a, dy, (const float2 *)stats, s.coef,
                       gamma, M, C, da);
    WSC_HIP(hipGetLastError());
    guard.free_now();
    return WSC_OK;
}

// ---- the per-op entries: the launchers of the pass unchanged -------------------------------------------------------------------
extern "C" {

int wsc_batch_norm_train_nhwc(wsc_ctx *ctx, const float *a_dev, long long M, int C, const float *gamma_dev, const float *beta_dev, float eps,
                              float keep, int unbiased, float *run_dev, float *stats_dev, float *y_dev) {
    WSC_CHECK(ctx && a_dev && gamma_dev && beta_dev && stats_dev && y_dev, WSC_ERR_INVALID, "wsc_batch_norm_train_nhwc: null argument");
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_batch_norm_train(ctx, a_dev, M, C, gamma_dev, beta_dev, eps, keep, unbiased, run_dev, stats_dev, y_dev);
}

int wsc_batch_norm_grad_nhwc(wsc_ctx *ctx, const float *a_dev, const float *stats_dev, const float *gamma_dev, const float *dy_dev, long long M,
                             int C, float *da_dev, float *dgamma_dev, float *dbeta_dev) {
    WSC_CHECK(ctx && a_dev && stats_dev && gamma_dev && dy_dev && da_dev && dgamma_dev && dbeta_dev, WSC_ERR_INVALID,
              "wsc_batch_norm_grad_nhwc: null argument");
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_batch_norm_grad(ctx, a_dev, stats_dev, gamma_dev, dy_dev, M, C, da_dev, dgamma_dev, dbeta_dev);
}

} // extern "C"
