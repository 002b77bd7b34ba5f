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
//   the last block of a slab to arrive (an integer ticket per slab: ticket_publish / ticket_is_last of common.h) adds
//   the partials in block order and finishes the slab's channels.
// No floating-point atomic, one fixed order: two calls give the same bits (on one device: the block count follows the CU count).
//   forward   the sums are of d = a - p and d d with the pivot p = a[0][c], formed in double (d is exact): mean = p + S / M,
//             var = Q / M - (S / M)^2 without the cancellation of sum a^2 / M - mean^2 (a channel of mean 1e3 and std 1e-2 keeps its
//             variance to double precision, a constant channel has var = 0 exactly)
//   backward  the sums are of dy and dy xh, xh = (a - mean) rstd in fp32 from the taped float statistics
// The file is compiled with the default contraction; the fused operations of the elementwise passes are spelled, and a - mean
// followed by a product cannot fuse, so the 16-byte form is the only form and every element takes the same roundings.
//
// The dropout sites of 01_train (the `D` entries of VGG16's layer5) sit BEHIND a BatchNorm, under the
// counter-based contract of dropout_rng.h:
//   forward   bn_apply_drop_*: one pass forms y = fma((a - mean) rstd, gamma, beta), drops and scales it in fp32 and stores it
//             ONCE into the net's activation type (fp32, or the hi / lo planes through the split and the range flag of the GroupNorm
//             store) together with the fp32 tape entry -- one rounding fewer than dropping the already split planes.  4 fp32 or 8
//             16-bit elements (one or two counter blocks) per thread, the loads issued before the ten rounds; a buffer off the
//             16-byte grid takes the scalar form, the same words.
//   backward  a kept BatchNorm output may be negative or exactly 0.0, so the tape cannot give the mask back: the DROP instantiations
//             of the two gradient kernels regenerate the keep bits from (seed, step, site) and replace dy ON LOAD by
//             keep ? fmul_rn(dy, scale) : +0.0 -- no mask buffer, no extra pass, the block geometry and the summation order of the
//             plain instantiations, which are the code of a pass without dropout.
#include "common.h"
#include "dropout_rng.h"

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
    DropRng rng;           // DROP: dy is the gradient BEHIND the dropout of y
};

// dy of elements 4 blk .. 4 blk + 3 as the BatchNorm's output sees it: the dropout's own gradient
__device__ __forceinline__ f32x4_t drop_dy(const DropRng &g, unsigned long long blk, f32x4_t d) {
    uint32_t w[4];
    drop_words(g, blk, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = drop_value(g, d[j], drop_keeps(g, w[j]));
    return d;
}

template <bool GRAD, bool DROP = false>
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
                f32x4_t d = *reinterpret_cast<const f32x4_t *>(a.dy + r * a.C + c0);
                if (DROP) d = drop_dy(a.rng, (unsigned long long)(r * a.C + c0) >> 2, d); // (C, c0 multiples of 4: one counter block)
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
        ticket_publish();
    }
    __syncthreads();
    if (tid == 0) s_last = ticket_is_last(a.tickets + slab, gridDim.x);
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

// ---- BatchNorm apply with dropout (the forward pass at a site) ------------------------------------------------------------------
constexpr int BN_DROP_BLOCK = 256;

struct BnDropArgs {
    const float *a;       // [M][C]
    const float2 *stats;  // [C] {mean, rstd}
    const float *gamma, *beta;
    long long n;          // M C elements
    int C;
    float *y;             // fp32 activation (WSC_PREC_F32), or null
    uint16_t *hi, *lo;    // 16-bit planes (lo null: one plane), or null
    int fmt;
    float *tape;          // the fp32 value the activation holds, or null
    unsigned *range;      // the ctx's range flag
    DropRng rng;
};

// elements 4 q .. 4 q + 3 are one counter block and channels c0 .. c0 + 3 of one row: what the block reads, loaded before the rounds
struct BnDropIn {
    f32x4_t v, ga, be;
    float2 st[4];
};
__device__ __forceinline__ BnDropIn bn_drop_load(const BnDropArgs &p, long long q) {
    const int c0 = (int)(q % (p.C >> 2)) * 4;
    BnDropIn in;
    in.v = *reinterpret_cast<const f32x4_t *>(p.a + 4 * q);
    in.ga = *reinterpret_cast<const f32x4_t *>(p.gamma + c0);
    in.be = *reinterpret_cast<const f32x4_t *>(p.beta + c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) in.st[j] = p.stats[c0 + j];
    return in;
}
// bn_apply_kernel's y of the block, dropped and scaled
__device__ __forceinline__ void bn_drop_group(const BnDropArgs &p, const BnDropIn &in, const uint32_t w[4], float d[4], bool *nan) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float y = __builtin_fmaf((in.v[j] - in.st[j].x) * in.st[j].y, in.ga[j], in.be[j]);
        *nan = *nan || y != y; // (a dropped NaN is still a NaN that entered the net)
        d[j] = drop_value(p.rng, y, drop_keeps(p.rng, w[j]));
    }
}
// the planes' halves of d by the GroupNorm store's split, the fp32 value they hold, whether an IEEE-half plane cannot hold d
__device__ __forceinline__ void bn_drop_split(float d, int fmt, bool split, uint16_t *h, uint16_t *l, float *held, bool *bad) {
    const uint16_t hh = f32_to_h16(d, fmt);
    float r = h16_to_f32(hh, fmt);
    uint16_t ll = 0;
    if (split) {
        ll = f32_to_h16(d - r, fmt); // the lo plane has the hi plane's format
        r = __fadd_rn(r, h16_to_f32(ll, fmt));
    }
    *h = hh; *l = ll; *held = r;
    *bad = *bad || (fmt == 1 && !(fabsf(d) < 65504.f));
}

// WSC_PREC_F32 (y) or the fp32 tape alone.  VEC: 4 elements = one counter block per thread, 16-byte accesses (n is a multiple of 4)
template <bool VEC>
__global__ __launch_bounds__(BN_DROP_BLOCK) void bn_apply_drop_f32_kernel(BnDropArgs p) {
    const long long t = (long long)blockIdx.x * BN_DROP_BLOCK + threadIdx.x;
    uint32_t w[4];
    if (!VEC) {
        if (t >= p.n) return;
        const int c = (int)(t % p.C);
        const float v = p.a[t];
        const float2 st = p.stats[c];
        const float ga = p.gamma[c], be = p.beta[c];
        drop_words(p.rng, (unsigned long long)t >> 2, w);
        const float d = drop_value(p.rng, __builtin_fmaf((v - st.x) * st.y, ga, be), drop_keeps(p.rng, w[t & 3]));
        if (p.y) p.y[t] = d;
        if (p.tape) p.tape[t] = d;
        return;
    }
    if (4 * t >= p.n) return;
    const BnDropIn in = bn_drop_load(p, t);
    drop_words(p.rng, (unsigned long long)t, w);
    float d[4];
    bool nan = false; // (fp32 carries a NaN through as a value)
    bn_drop_group(p, in, w, d, &nan);
    const f32x4_t o = {d[0], d[1], d[2], d[3]};
    if (p.y) *reinterpret_cast<f32x4_t *>(p.y + 4 * t) = o;
    if (p.tape) *reinterpret_cast<f32x4_t *>(p.tape + 4 * t) = o;
}

// the 16-bit planes.  VEC: 8 elements = 16 bytes of a plane and two counter blocks per thread (n a multiple of 4: the last thread
// may own one block)
template <bool VEC>
__global__ __launch_bounds__(BN_DROP_BLOCK) void bn_apply_drop_h16_kernel(BnDropArgs p) {
    const long long t = (long long)blockIdx.x * BN_DROP_BLOCK + threadIdx.x;
    const bool split = p.lo != nullptr;
    bool bad = false;
    if (!VEC) {
        if (t < p.n) {
            const int c = (int)(t % p.C);
            const float v = p.a[t];
            const float2 st = p.stats[c];
            const float ga = p.gamma[c], be = p.beta[c];
            uint32_t w[4];
            drop_words(p.rng, (unsigned long long)t >> 2, w);
            const float y = __builtin_fmaf((v - st.x) * st.y, ga, be);
            uint16_t h, l;
            float held;
            bn_drop_split(drop_value(p.rng, y, drop_keeps(p.rng, w[t & 3])), p.fmt, split, &h, &l, &held, &bad);
            bad = bad || (p.fmt == 1 && y != y);
            p.hi[t] = h;
            if (split) p.lo[t] = l;
            if (p.tape) p.tape[t] = held;
        }
    } else if (8 * t < p.n) {
        const long long base = 8 * t;
        const bool two = base + 8 <= p.n;
        const BnDropIn in0 = bn_drop_load(p, 2 * t), in1 = bn_drop_load(p, two ? 2 * t + 1 : 2 * t);
        uint32_t w[8];
        drop_words(p.rng, 2ull * (unsigned long long)t, w);
        drop_words(p.rng, 2ull * (unsigned long long)t + 1, w + 4);
        float d[8] = {};
        bool nan = false;
        bn_drop_group(p, in0, w, d, &nan);
        if (two) bn_drop_group(p, in1, w + 4, d + 4, &nan);
        bad = p.fmt == 1 && nan;
        uint16_t ho[8], lw[8];
        float held[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            bool b = false;
            bn_drop_split(d[e], p.fmt, split, &ho[e], &lw[e], &held[e], &b);
            if (e < 4 || two) bad = bad || b;
        }
        auto pk = [](uint16_t a, uint16_t b) { return (uint32_t)a | ((uint32_t)b << 16); };
        if (two) {
            *reinterpret_cast<uint4 *>(p.hi + base) = make_uint4(pk(ho[0], ho[1]), pk(ho[2], ho[3]), pk(ho[4], ho[5]), pk(ho[6], ho[7]));
            if (split) *reinterpret_cast<uint4 *>(p.lo + base) = make_uint4(pk(lw[0], lw[1]), pk(lw[2], lw[3]), pk(lw[4], lw[5]), pk(lw[6], lw[7]));
        } else {
            *reinterpret_cast<uint2 *>(p.hi + base) = make_uint2(pk(ho[0], ho[1]), pk(ho[2], ho[3]));
            if (split) *reinterpret_cast<uint2 *>(p.lo + base) = make_uint2(pk(lw[0], lw[1]), pk(lw[2], lw[3]));
        }
        if (p.tape) {
            *reinterpret_cast<float4 *>(p.tape + base) = make_float4(held[0], held[1], held[2], held[3]);
            if (two) *reinterpret_cast<float4 *>(p.tape + base + 4) = make_float4(held[4], held[5], held[6], held[7]);
        }
    }
    if (bad) *p.range = (unsigned)p.C; // (a plain store of a non-zero value: every writer writes "raised")
}

// da = (gamma rstd) ((dy - mb) - xh mg), {mb, mg} = coef: every product and difference one fp32 rounding, xh mg fused into the
// second difference.  DROP: dy through drop_dy first, as in the sums
template <bool DROP>
__global__ __launch_bounds__(256) void bn_grad_apply_kernel(const float *__restrict__ a, const float *__restrict__ dy,
                                                            const float2 *__restrict__ stats, const float2 *__restrict__ coef,
                                                            const float *__restrict__ gamma, long long M, int C, float *__restrict__ da,
                                                            DropRng rng) {
    const int C4 = C >> 2;
    const long long total = M * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % C4) * 4;
        const f32x4_t v = *reinterpret_cast<const f32x4_t *>(a + i * 4);
        f32x4_t d = *reinterpret_cast<const f32x4_t *>(dy + i * 4), o;
        if (DROP) d = drop_dy(rng, (unsigned long long)i, d);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 st = stats[c0 + j], cf = coef[c0 + j];
            const float xh = (v[j] - st.x) * st.y;
            o[j] = (gamma[c0 + j] * st.y) * __builtin_fmaf(-xh, cf.y, d[j] - cf.x);
        }
        *reinterpret_cast<f32x4_t *>(da + i * 4) = o;
    }
}

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

int launch_batch_norm_apply_drop(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *beta, long long M, int C,
                                 Act act, float *tape, float drop_prob, unsigned long long seed, unsigned step, unsigned site) {
    WSC_TRY(bn_shape_check("BatchNorm with dropout", M, C));
    WSC_CHECK(aligned16(a) && ((uintptr_t)stats & 7u) == 0, WSC_ERR_INVALID, "BatchNorm with dropout: a must be 16-byte aligned, stats 8-byte aligned");
    BnDropArgs p = {};
    p.a = a; p.stats = (const float2 *)stats; p.gamma = gamma; p.beta = beta;
    p.n = M * C; p.C = C;
    const bool f32 = act.is_f32();
    if (f32) p.y = act.f32();
    else { p.hi = act.h16(); p.lo = act.h16_lo(); }
    p.fmt = act.fmt();
    p.tape = tape;
    p.range = ctx->range_dev;
    p.rng = drop_rng(drop_prob, seed, step, site);
    const bool vec = aligned16(gamma) && aligned16(beta) && aligned16(act.hi) && aligned16(act.lo) && aligned16(tape);
    const long long blocks = ((p.n + (vec ? (f32 ? 4 : 8) : 1) - 1) / (vec ? (f32 ? 4 : 8) : 1) + BN_DROP_BLOCK - 1) / BN_DROP_BLOCK;
    WSC_CHECK(blocks < (1ll << 31), WSC_ERR_INVALID, "BatchNorm with dropout: %lld elements", p.n);
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (double)p.n * (4 + (f32 ? 4 : (p.lo ? 4 : 2)) + (tape ? 4 : 0)));
    const dim3 grid((unsigned)blocks), block(BN_DROP_BLOCK);
    if (f32 && vec) hipLaunchKernelGGL(bn_apply_drop_f32_kernel<true>, grid, block, 0, ctx->stream, p);
    else if (f32) hipLaunchKernelGGL(bn_apply_drop_f32_kernel<false>, grid, block, 0, ctx->stream, p);
    else if (vec) hipLaunchKernelGGL(bn_apply_drop_h16_kernel<true>, grid, block, 0, ctx->stream, p);
    else hipLaunchKernelGGL(bn_apply_drop_h16_kernel<false>, grid, block, 0, ctx->stream, p);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

namespace {
// rng null: the plain instantiations
int bn_grad_launch(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *dy, long long M, int C, float *da,
                   float *dgamma, float *dbeta, const DropRng *rng) {
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
    if (rng) s.rng = *rng;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 20.0 * M * C);
    const dim3 sums(sc.blocks, sc.slabs), apply(wsc_grid_for(M * (C / 4)));
    if (rng) hipLaunchKernelGGL((bn_sums_kernel<true, true>), sums, dim3(BN_BLOCK), 0, ctx->stream, s);
    else hipLaunchKernelGGL((bn_sums_kernel<true>), sums, dim3(BN_BLOCK), 0, ctx->stream, s);
    WSC_HIP(hipGetLastError());
    if (rng)
        hipLaunchKernelGGL(bn_grad_apply_kernel<true>, apply, dim3(256), 0, ctx->stream, a, dy, (const float2 *)stats, s.coef, gamma, M, C, da, s.rng);
    else
        hipLaunchKernelGGL(bn_grad_apply_kernel<false>, apply, dim3(256), 0, ctx->stream, a, dy, (const float2 *)stats, s.coef, gamma, M, C, da, s.rng);
    WSC_HIP(hipGetLastError());
    guard.free_now();
    return WSC_OK;
}
} // namespace

int launch_batch_norm_grad(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *dy, long long M, int C,
                           float *da, float *dgamma, float *dbeta) {
    return bn_grad_launch(ctx, a, stats, gamma, dy, M, C, da, dgamma, dbeta, nullptr);
}

int launch_batch_norm_grad_drop(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *dy, long long M, int C,
                                float *da, float *dgamma, float *dbeta, float drop_prob, unsigned long long seed, unsigned step, unsigned site) {
    const DropRng rng = drop_rng(drop_prob, seed, step, site);
    return bn_grad_launch(ctx, a, stats, gamma, dy, M, C, da, dgamma, dbeta, &rng);
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

int wsc_batch_norm_train_drop_nhwc(wsc_ctx *ctx, const float *a_dev, long long M, int C, const float *gamma_dev, const float *beta_dev, float eps,
                                   float keep, int unbiased, float *run_dev, float *stats_dev, float *y_dev, float drop_prob,
                                   unsigned long long seed, long long step, int site) {
    const char *fn = "wsc_batch_norm_train_drop_nhwc";
    WSC_CHECK(ctx && a_dev && gamma_dev && beta_dev && stats_dev && y_dev, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_TRY(seg_dropout_check(fn, drop_prob, step));
    WSC_CHECK(site >= 0 && ((uintptr_t)y_dev & 3u) == 0, WSC_ERR_INVALID, "%s: site %d, or y_dev is not 4-byte aligned", fn, site);
    WSC_HIP(hipSetDevice(ctx->device));
    WSC_TRY(launch_batch_norm_train(ctx, a_dev, M, C, gamma_dev, beta_dev, eps, keep, unbiased, run_dev, stats_dev, nullptr));
    Act y;
    y.prec = WSC_PREC_F32;
    y.hi = y_dev;
    return launch_batch_norm_apply_drop(ctx, a_dev, stats_dev, gamma_dev, beta_dev, M, C, y, nullptr, drop_prob, seed, (unsigned)step, (unsigned)site);
}

int wsc_batch_norm_grad_drop_nhwc(wsc_ctx *ctx, const float *a_dev, const float *stats_dev, const float *gamma_dev, const float *dy_dev,
                                  long long M, int C, float *da_dev, float *dgamma_dev, float *dbeta_dev, float drop_prob,
                                  unsigned long long seed, long long step, int site) {
    const char *fn = "wsc_batch_norm_grad_drop_nhwc";
    WSC_CHECK(ctx && a_dev && stats_dev && gamma_dev && dy_dev && da_dev && dgamma_dev && dbeta_dev, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_TRY(seg_dropout_check(fn, drop_prob, step));
    WSC_CHECK(site >= 0, WSC_ERR_INVALID, "%s: site %d", fn, site);
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_batch_norm_grad_drop(ctx, a_dev, stats_dev, gamma_dev, dy_dev, M, C, da_dev, dgamma_dev, dbeta_dev, drop_prob, seed,
                                       (unsigned)step, (unsigned)site);
}

} // extern "C"
