// seg_sgd.hip -- the update half of a SEC / DSRG training step (Model.optimize(), model.py:379-404) on the flat fp32 layout of
// wsc_seg_grad_layout, and the device repack that brings the updated floats into a net (wsc_seg_sgd_accumulate, wsc_seg_sgd_apply,
// wsc_net_seg_load_params of net.hip).  Built with -ffp-contract=off: every product, sum and quotient below is one fp32 rounding.
//
//   accumulate   t = grad + wd param (weights), t = grad (biases); t = mult t; accum += t / accum_num.  One thread per 16-byte vector
//                of the WHOLE buffer: the layers' offsets are any (a 5-class fc8 bias makes every later one odd), so a vector may
//                straddle segments; an element's segment is found by bisection of the table (in LDS) for the vector's first float
//                and stepped forward per element.  A buffer that is not 16-byte aligned takes the scalar form of the same kernel.
//                loss["l2"] = sum w^2 / 2: per thread in double over its grid-stride elements, a fixed LDS tree per block, the
//                block partials to HBM; the block that arrives last (an integer ticket, agent-scope release / acquire) adds the
//                partials in block order and rounds once.  No floating-point atomic: two calls give the same bits.
//   apply        mom = mom momentum + accum; param = param - lr mom; accum = +0.0 (clear): three streams in, three out.
//   repack       HWIO has Cout fastest, the packed rows K fastest: a transpose.  Per K-step (one tap of one channel chunk) a
//                block moves a [ck channels][64 output channels] tile through LDS: rows of 256 bytes in, and out 16 bytes per
//                lane with ck / 8 adjacent lanes on one row's 128-byte K-step (hi | lo of the interleaved layout included).  The
//                per-channel maximum of the IEEE-half modes is a column reduction with the lanes along Cout, split over row
//                ranges into partial maxima the pack blocks finish (a maximum is exact in any order).  The rotated kernel of the
//                data gradient keeps 32 output channels contiguous: a gather copy, one thread per output float.
//                The first layer (Cin = 3 in a 4-channel slot, 27 weights per channel) has a small kernel of its own.
//                The IRNet heads (wsc_net_irn_load_params) come through the same jobs at k = 1: a job without a bias (b_off < 0)
//                gets b1 = 0, and one whose input is wider than its tensor (Cin_pad: the final edge conv, 160 in 192) packs
//                zeros for the channels past Cin; a DeepLab job has neither, and its bits and launches are what they were.
//                Four launches for the whole net, whatever its depth: each kernel finds its layer in a device table of per-layer
//                jobs built once per wsc_seg_grad (a launch per layer and kernel was launch-bound: ~10 us each, 75 of them).
#include "common.h"

#include <algorithm>

namespace {

constexpr int SGD_BLOCK = 256;
constexpr int SGD_PMAX_SPLITS = 64; // row ranges of a layer's partial channel maxima, at most

struct SgdAccArgs {
    const SgdSegment *segs;
    int n_segs;
    const float *param, *grad;
    float *accum;
    long long elems;
    float wd, div;
    double *partials; // null: no l2
    unsigned *counter;
    float *l2;
};

__device__ __forceinline__ float sgd_acc_one(float p, float g, float a, float wd, float mult, int decay, float div) {
    float t = g;
    if (decay) t = __fadd_rn(g, __fmul_rn(wd, p));
    t = __fmul_rn(mult, t);
    return __fadd_rn(a, __fdiv_rn(t, div));
}

template <bool VEC>
__global__ __launch_bounds__(SGD_BLOCK) void sgd_accumulate_kernel(SgdAccArgs a) {
    __shared__ long long s_start[SGD_MAX_SEGMENTS + 1];
    __shared__ float s_mult[SGD_MAX_SEGMENTS];
    __shared__ int s_decay[SGD_MAX_SEGMENTS];
    __shared__ double red[SGD_BLOCK], fin[SGD_L2_MAX_BLOCKS];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    for (int i = tid; i < a.n_segs; i += SGD_BLOCK) {
        s_start[i] = a.segs[i].start;
        s_mult[i] = a.segs[i].mult;
        s_decay[i] = a.segs[i].decay;
    }
    if (tid == 0) s_start[a.n_segs] = a.elems;
    __syncthreads();

    const bool want_l2 = a.partials != nullptr;
    double sq = 0.0;
    constexpr int PER = VEC ? 4 : 1;
    const long long nvec = (a.elems + PER - 1) / PER;
    for (long long v = (long long)blockIdx.x * SGD_BLOCK + tid; v < nvec; v += (long long)gridDim.x * SGD_BLOCK) {
        const long long base = v * PER;
        int seg = 0, hi = a.n_segs - 1; // the last segment that starts at or before `base`
        while (seg < hi) {
            const int mid = (seg + hi + 1) >> 1;
            if (s_start[mid] <= base) seg = mid;
            else hi = mid - 1;
        }
        if (VEC && base + 4 <= a.elems) {
            const float4 p4 = *reinterpret_cast<const float4 *>(a.param + base);
            const float4 g4 = *reinterpret_cast<const float4 *>(a.grad + base);
            const float4 a4 = *reinterpret_cast<const float4 *>(a.accum + base);
            const float p[4] = {p4.x, p4.y, p4.z, p4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w}, ac[4] = {a4.x, a4.y, a4.z, a4.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                while (base + e >= s_start[seg + 1]) ++seg; // (a boundary inside the vector; s_start[n_segs] = elems ends it)
                const int decay = s_decay[seg];
                o[e] = sgd_acc_one(p[e], g[e], ac[e], a.wd, s_mult[seg], decay, a.div);
                if (want_l2 && decay) sq += (double)p[e] * (double)p[e];
            }
            *reinterpret_cast<float4 *>(a.accum + base) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            for (long long i = base; i < base + PER && i < a.elems; ++i) {
                while (i >= s_start[seg + 1]) ++seg;
                const int decay = s_decay[seg];
                const float p = a.param[i];
                a.accum[i] = sgd_acc_one(p, a.grad[i], a.accum[i], a.wd, s_mult[seg], decay, a.div);
                if (want_l2 && decay) sq += (double)p * (double)p;
            }
        }
    }
    if (!want_l2) return; // (block-uniform)

    red[tid] = sq;
    __syncthreads();
    for (int s = SGD_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        a.partials[blockIdx.x] = red[0];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == gridDim.x - 1;
        if (s_last) { // every block's partial is out
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    // the finishing block: the partials come in side by side, thread 0 adds them in block order
    for (unsigned b = tid; b < gridDim.x; b += SGD_BLOCK) fin[b] = a.partials[b];
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) s += fin[b];
        *a.l2 = (float)(0.5 * s);
    }
}

template <bool VEC>
__global__ __launch_bounds__(SGD_BLOCK) void sgd_apply_kernel(float *param, float *accum, float *mom, long long elems, float lr, float momentum,
                                                              int clear) {
    constexpr int PER = VEC ? 4 : 1;
    const long long nvec = (elems + PER - 1) / PER;
    for (long long v = (long long)blockIdx.x * SGD_BLOCK + threadIdx.x; v < nvec; v += (long long)gridDim.x * SGD_BLOCK) {
        const long long base = v * PER;
        if (VEC && base + 4 <= elems) {
            const float4 p4 = *reinterpret_cast<const float4 *>(param + base);
            const float4 a4 = *reinterpret_cast<const float4 *>(accum + base);
            const float4 m4 = *reinterpret_cast<const float4 *>(mom + base);
            float4 m, p;
            m.x = __fadd_rn(__fmul_rn(m4.x, momentum), a4.x); p.x = __fsub_rn(p4.x, __fmul_rn(lr, m.x));
            m.y = __fadd_rn(__fmul_rn(m4.y, momentum), a4.y); p.y = __fsub_rn(p4.y, __fmul_rn(lr, m.y));
            m.z = __fadd_rn(__fmul_rn(m4.z, momentum), a4.z); p.z = __fsub_rn(p4.z, __fmul_rn(lr, m.z));
            m.w = __fadd_rn(__fmul_rn(m4.w, momentum), a4.w); p.w = __fsub_rn(p4.w, __fmul_rn(lr, m.w));
            *reinterpret_cast<float4 *>(mom + base) = m;
            *reinterpret_cast<float4 *>(param + base) = p;
            if (clear) *reinterpret_cast<float4 *>(accum + base) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (long long i = base; i < base + PER && i < elems; ++i) {
                const float m = __fadd_rn(__fmul_rn(mom[i], momentum), accum[i]);
                mom[i] = m;
                param[i] = __fsub_rn(param[i], __fmul_rn(lr, m));
                if (clear) accum[i] = 0.f;
            }
        }
    }
}

int sgd_blocks(long long elems, bool vec) {
    const long long nvec = vec ? (elems + 3) / 4 : elems;
    return (int)std::min<long long>(std::max<long long>((nvec + SGD_BLOCK - 1) / SGD_BLOCK, 1), SGD_L2_MAX_BLOCKS);
}

// ---- repack -----------------------------------------------------------------------------------------------------------------------
// Every kernel below is ONE launch over all layers: block b belongs to the layer whose block range holds it (the table's
// *_block0, in layer order; a layer without blocks in a launch has an empty range).
#define REPACK_FIND_JOB(field)                                                        \
    int ji = 0;                                                                       \
    while (ji + 1 < n_jobs && (int)blockIdx.x >= jobs[ji + 1].field) ++ji;            \
    const RepackJob &J = jobs[ji];                                                    \
    const int lb = (int)blockIdx.x - J.field /* the block's index inside the layer */

// pmax[split][c] = max |w[r][c]| over the split's rows (a NaN is passed over, as std::max passes it over in make_conv: the pack
// kernels below raise the range flag for it);
// block (tile, split) of a layer = lb % tiles, lb / tiles
__global__ __launch_bounds__(256) void repack_colmax_kernel(const RepackJob *__restrict__ jobs, int n_jobs, const float *__restrict__ param,
                                                            float *__restrict__ pmax_all) {
    __shared__ float red[4][64];
    REPACK_FIND_JOB(max_block0);
    const float *w = param + J.w_off;
    float *pmax = pmax_all + J.pmax_off;
    const int Cout = J.Cout, R = J.k * J.k * J.Cin;
    const int tile = lb % J.tiles, split = lb / J.tiles;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = tile * 64 + lane;
    const int r0 = split * J.rows_per, r1 = min(r0 + J.rows_per, R);
    float m = 0.f;
    if (c < Cout) {
#pragma unroll 4
        for (int r = r0 + wv; r < r1; r += 4) m = fmaxf(m, fabsf(w[(long long)r * Cout + c]));
    }
    red[wv][lane] = m;
    __syncthreads();
    if (wv == 0 && c < Cout) pmax[(long long)split * Cout + c] = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
}

constexpr int REPACK_STEPS = 4; // K-steps per block

__device__ __forceinline__ unsigned pack2(uint16_t a, uint16_t b) { return (unsigned)a | ((unsigned)b << 16); }

// block (x, y) of a layer = (lb % tiles, lb / tiles): output channels [64 x, 64 x + 64), K-steps [REPACK_STEPS y, ...); K-step
// (cc, r, s) = CK channels of tap (r, s).  fmt / split: conv_fmt / conv_split != 0 of the net's precision.
template <int CK>
__global__ __launch_bounds__(256) void repack_generic_kernel(const RepackJob *__restrict__ jobs, int n_jobs, const float *__restrict__ param,
                                                             const float *__restrict__ pmax_all, int fmt, int split, unsigned *range) {
    constexpr int LD = 65, G = CK / 8;
    // the door of the range guard for what the device packs (make_conv's for the host): a weight or bias that is not finite raises
    // the ctx's flag, in every precision -- the step that made it has diverged, and the half formats cannot hold it at all
    bool bad = false;
    __shared__ float tile[CK][LD];
    __shared__ float s_scale[64];
    REPACK_FIND_JOB(pack_block0);
    const float *w = param + J.w_off;
    const int Cout = J.Cout, Cin = J.Cin, k = J.k, Kw = J.Kw, kstep = J.kstep;
    const int bx = lb % J.tiles, by = lb / J.tiles;
    const int tid = threadIdx.x;
    const int co0 = bx * 64;
    if (tid < 64) {
        const int c = co0 + tid;
        float scale = 1.f, inv = 1.f;
        if (c < Cout) {
            if (fmt == 1) {
                const float *pmax = pmax_all + J.pmax_off;
                float mx = 0.f;
                for (int s = 0; s < J.splits; ++s) mx = fmaxf(mx, pmax[(long long)s * Cout + c]);
                const int sh = conv_half_shift(mx);
                scale = conv_pow2(sh);
                inv = conv_pow2(-sh);
            }
            if (by == 0) {
                J.s1[c] = inv;
                J.b1[c] = J.b_off >= 0 ? param[J.b_off + c] : 0.f;
                bad = !(fabsf(J.b1[c]) < INFINITY);
            }
        }
        s_scale[tid] = scale;
    }
    const int ks0 = by * REPACK_STEPS, ks1 = min(ks0 + REPACK_STEPS, J.nsteps);
    for (int ks = ks0; ks < ks1; ++ks) {
        const int s = ks % k, r = (ks / k) % k, cc = ks / (k * k);
        const float *src = w + ((long long)(r * k + s) * Cin + cc * CK) * Cout + co0;
        __syncthreads(); // (the previous tile is read; s_scale is written)
#pragma unroll
        for (int i = 0; i < CK / 4; ++i) {
            const int row = (tid >> 6) + 4 * i, col = tid & 63;
            const float wv = co0 + col < Cout && cc * CK + row < Cin ? src[(long long)row * Cout + col] : 0.f; // (Cin_pad: zeros past Cin)
            tile[row][col] = wv;
            bad = bad || !(fabsf(wv) < INFINITY);
        }
        __syncthreads();
        for (int j = tid; j < 64 * G; j += 256) {
            const int co = j / G, grp = j - co * G;
            const int c = co0 + co;
            if (c >= Cout) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = tile[grp * 8 + e][co];
            const long long at = (long long)c * Kw + (long long)ks * kstep + grp * 8;
            if (fmt == CONV_FMT_F32) {
                float4 *dst = reinterpret_cast<float4 *>((float *)J.wp + at);
                dst[0] = make_float4(v[0], v[1], v[2], v[3]);
                dst[1] = make_float4(v[4], v[5], v[6], v[7]);
                continue;
            }
            const float sc = s_scale[co];
            uint16_t h[8], l[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = v[e] * sc;
                h[e] = f32_to_h16(x, fmt);
                l[e] = f32_to_h16(x - h16_to_f32(h[e], fmt), fmt);
            }
            uint16_t *row = (uint16_t *)J.wp + at;
            *reinterpret_cast<uint4 *>(row) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
            if (split)
                *reinterpret_cast<uint4 *>(row + J.lo_at) = make_uint4(pack2(l[0], l[1]), pack2(l[2], l[3]), pack2(l[4], l[5]), pack2(l[6], l[7]));
        }
    }
    if (bad) *range = (unsigned)Cout;
}

// the first layer: CONV_FORM_SMALL2, weight (ci, r, s) at r 16 + s 4 + ci of its row; one thread per output channel
__global__ __launch_bounds__(64) void repack_small2_kernel(const RepackJob *__restrict__ jobs, int job, const float *__restrict__ param, int fmt,
                                                           int split, unsigned *range) {
    const RepackJob &J = jobs[job];
    const float *w = param + J.w_off;
    const int Cout = J.Cout;
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= Cout) return;
    const int n = J.k * J.k * J.Cin;
    float scale = 1.f, inv = 1.f;
    if (fmt == 1) {
        float mx = 0.f;
        for (int i = 0; i < n; ++i) mx = fmaxf(mx, fabsf(w[(long long)i * Cout + c]));
        const int sh = conv_half_shift(mx);
        scale = conv_pow2(sh);
        inv = conv_pow2(-sh);
    }
    J.s1[c] = inv;
    J.b1[c] = param[J.b_off + c];
    bool bad = !(fabsf(J.b1[c]) < INFINITY); // (the door, as repack_generic_kernel's)
    for (int i = 0; i < n; ++i) {
        const int ci = i % J.Cin, s = (i / J.Cin) % J.k, r = i / (J.Cin * J.k);
        const float v = w[(long long)i * Cout + c];
        bad = bad || !(fabsf(v) < INFINITY);
        const long long at = (long long)c * J.Kw + r * 16 + s * 4 + ci;
        if (fmt == CONV_FMT_F32) {
            ((float *)J.wp)[at] = v;
            continue;
        }
        const float x = v * scale;
        const uint16_t h = f32_to_h16(x, fmt);
        ((uint16_t *)J.wp)[at] = h;
        if (split) ((uint16_t *)J.wp)[at + J.lo_at] = f32_to_h16(x - h16_to_f32(h, fmt), fmt);
    }
    if (bad) *range = (unsigned)Cout;
}

// rot[ci][((co / 32) k + r) k + s][co % 32] = w[k - 1 - r][k - 1 - s][ci][co], co < Cout (the floats past Cout keep their zeros);
// one thread per output float, a grid-stride loop over the layer's blocks
__global__ __launch_bounds__(256) void repack_rot_kernel(const RepackJob *__restrict__ jobs, int n_jobs, const float *__restrict__ param) {
    REPACK_FIND_JOB(rot_block0);
    const int nb = (ji + 1 < n_jobs ? jobs[ji + 1].rot_block0 : (int)gridDim.x) - J.rot_block0;
    const float *w = param + J.w_off;
    float *rot = J.w_rot;
    const int k = J.k, Cin = J.Cin, Cout = J.Cout, Kw = J.rot_Kw;
    const long long total = (long long)Cin * Kw;
    for (long long o = (long long)lb * 256 + threadIdx.x; o < total; o += (long long)nb * 256) {
        const int ci = (int)(o / Kw), rem = (int)(o - (long long)ci * Kw);
        const int c32 = rem & 31, t = rem >> 5;
        const int s = t % k, r = (t / k) % k, cq = t / (k * k);
        const int co = cq * 32 + c32;
        if (co < Cout) rot[o] = w[(((long long)(k - 1 - r) * k + (k - 1 - s)) * Cin + ci) * Cout + co];
    }
}

} // namespace

int sgd_accumulate_launch(wsc_ctx *ctx, const SgdSegment *segs_dev, int n_segs, const float *param, const float *grad, float *accum,
                          long long elems, float weight_decay, int accum_num, double *l2_partials, unsigned *l2_counter, float *l2_dev) {
    WSC_CHECK(n_segs >= 1 && n_segs <= SGD_MAX_SEGMENTS, WSC_ERR_INVALID, "internal: %d segments", n_segs);
    SgdAccArgs a = {};
    a.segs = segs_dev; a.n_segs = n_segs;
    a.param = param; a.grad = grad; a.accum = accum;
    a.elems = elems;
    a.wd = weight_decay; a.div = (float)accum_num;
    a.partials = l2_dev ? l2_partials : nullptr;
    a.counter = l2_counter; a.l2 = l2_dev;
    const bool vec = aligned16(param) && aligned16(grad) && aligned16(accum);
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 16.0 * elems);
    if (l2_dev) WSC_HIP(hipMemsetAsync(l2_counter, 0, sizeof(unsigned), ctx->stream)); // (the ticket starts at zero whatever came before)
    if (vec) hipLaunchKernelGGL(sgd_accumulate_kernel<true>, dim3(sgd_blocks(elems, true)), dim3(SGD_BLOCK), 0, ctx->stream, a);
    else hipLaunchKernelGGL(sgd_accumulate_kernel<false>, dim3(sgd_blocks(elems, false)), dim3(SGD_BLOCK), 0, ctx->stream, a);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int sgd_apply_launch(wsc_ctx *ctx, float *param, float *accum, float *mom, long long elems, float lr, float momentum, int clear_accum) {
    const bool vec = aligned16(param) && aligned16(accum) && aligned16(mom);
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (clear_accum ? 24.0 : 20.0) * elems);
    if (vec)
        hipLaunchKernelGGL(sgd_apply_kernel<true>, dim3(sgd_blocks(elems, true)), dim3(SGD_BLOCK), 0, ctx->stream, param, accum, mom, elems, lr,
                           momentum, clear_accum);
    else
        hipLaunchKernelGGL(sgd_apply_kernel<false>, dim3(sgd_blocks(elems, false)), dim3(SGD_BLOCK), 0, ctx->stream, param, accum, mom, elems, lr,
                           momentum, clear_accum);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int repack_plan(std::vector<RepackJob> &jobs, wsc_precision prec, RepackPlan *plan) {
    *plan = RepackPlan();
    plan->prec = prec;
    plan->n_jobs = (int)jobs.size();
    const int fmt = conv_fmt(prec);
    for (size_t i = 0; i < jobs.size(); ++i) {
        RepackJob &J = jobs[i];
        WSC_CHECK(!J.small || (J.Cin <= 4 && J.k <= 4 && plan->small_job < 0), WSC_ERR_INVALID, "internal: repack of a small-Cin layer %d x %d x %d",
                  J.k, J.k, J.Cin); // (one such layer, the first)
        const int cin_lay = J.Cin_pad ? J.Cin_pad : J.Cin; // the channels of the packed rows
        WSC_CHECK(J.Cin_pad == 0 || (!J.small && J.k == 1 && J.Cin_pad >= J.Cin), WSC_ERR_INVALID,
                  "internal: repack of %d x %d x %d into rows of %d channels", J.k, J.k, J.Cin, J.Cin_pad); // (a padded input: 1 x 1 layers)
        const ConvKLayout lay = conv_k_layout(J.k, J.k, J.small ? 4 : cin_lay, J.small ? CONV_FORM_SMALL2 : CONV_FORM_GENERIC, prec);
        WSC_CHECK(J.small || (cin_lay % lay.ck == 0 && (lay.ck == 32 || lay.ck == 64)), WSC_ERR_INVALID, "internal: repack of Cin=%d in chunks of %d",
                  cin_lay, lay.ck);
        if (!J.small) plan->ck = lay.ck; // (the precision's: one value for every generic layer)
        J.kstep = lay.kstep; J.Kw = lay.Kw; J.lo_at = lay.lo_at; J.nsteps = lay.ksteps_base;
        J.rot_Kw = J.w_rot ? J.k * J.k * dgrad_cz(J.Cout) : 0;
        J.tiles = (J.Cout + 63) / 64;
        const int R = J.k * J.k * J.Cin;
        J.splits = 0; J.rows_per = R; J.pmax_off = 0;
        J.max_block0 = plan->max_blocks; J.pack_block0 = plan->pack_blocks; J.rot_block0 = plan->rot_blocks;
        if (J.small) {
            plan->small_job = (int)i;
            plan->small_tiles = (J.Cout + 63) / 64;
        } else {
            if (fmt == 1) { // the partial maxima: ~512 blocks a layer, at least 16 rows each
                int splits = std::max(1, std::min(std::min(512 / J.tiles, SGD_PMAX_SPLITS), (R + 15) / 16));
                J.rows_per = (R + splits - 1) / splits;
                J.splits = (R + J.rows_per - 1) / J.rows_per; // (no empty split)
                J.pmax_off = plan->pmax_elems;
                plan->pmax_elems += (long long)J.splits * J.Cout;
                plan->max_blocks += J.tiles * J.splits;
            }
            plan->pack_blocks += J.tiles * ((J.nsteps + REPACK_STEPS - 1) / REPACK_STEPS);
        }
        if (J.w_rot) plan->rot_blocks += wsc_grid_for((long long)J.Cin * J.rot_Kw);
        plan->bytes += 4.0 * R * J.Cout * 2 + (double)J.Cout * lay.Kw * conv_elem_bytes(prec) + (J.w_rot ? 4.0 * R * J.Cout : 0.0);
    }
    return WSC_OK;
}

int repack_launch(wsc_ctx *ctx, const RepackPlan &plan, const float *param) {
    const int fmt = conv_fmt(plan.prec), split = conv_split(plan.prec) != 0;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, plan.bytes);
    // (wsc_ctx_scratch_fill: the partial maxima are scratch of this call, kept by the grad object between calls)
    if (ctx->scratch_fill >= 0 && plan.pmax) WSC_HIP(hipMemsetAsync(plan.pmax, ctx->scratch_fill, (size_t)plan.pmax_elems * sizeof(float), ctx->stream));
    if (plan.max_blocks > 0) {
        hipLaunchKernelGGL(repack_colmax_kernel, dim3(plan.max_blocks), dim3(256), 0, ctx->stream, plan.jobs_dev, plan.n_jobs, param, plan.pmax);
        WSC_HIP(hipGetLastError());
    }
    if (plan.pack_blocks > 0) {
        if (plan.ck == 32)
            hipLaunchKernelGGL(repack_generic_kernel<32>, dim3(plan.pack_blocks), dim3(256), 0, ctx->stream, plan.jobs_dev, plan.n_jobs, param,
                               plan.pmax, fmt, split, ctx->range_dev);
        else
            hipLaunchKernelGGL(repack_generic_kernel<64>, dim3(plan.pack_blocks), dim3(256), 0, ctx->stream, plan.jobs_dev, plan.n_jobs, param,
                               plan.pmax, fmt, split, ctx->range_dev);
        WSC_HIP(hipGetLastError());
    }
    if (plan.small_job >= 0) {
        hipLaunchKernelGGL(repack_small2_kernel, dim3(plan.small_tiles), dim3(64), 0, ctx->stream, plan.jobs_dev, plan.small_job, param, fmt, split, ctx->range_dev);
        WSC_HIP(hipGetLastError());
    }
    if (plan.rot_blocks > 0) {
        hipLaunchKernelGGL(repack_rot_kernel, dim3(plan.rot_blocks), dim3(256), 0, ctx->stream, plan.jobs_dev, plan.n_jobs, param);
        WSC_HIP(hipGetLastError());
    }
    return WSC_OK;
}
