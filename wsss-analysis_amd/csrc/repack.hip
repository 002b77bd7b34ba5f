// repack.hip -- the device repack that brings the floats of a flat fp32 parameter buffer, as an optimiser step of sgd.hip leaves
// them, into a net: what wsc_net_seg_load_params, wsc_net_irn_load_params and wsc_net_cls_load_params of net.hip launch.  Built
// with -ffp-contract=off, and the BatchNorm fold's operations are spelled with their round-to-nearest intrinsics: one rounding each.
//
//   conv rows    HWIO has Cout fastest, the packed rows K fastest: a transpose.  Per K-step (one tap of one channel chunk) a
//                block moves a [ck channels][64 output channels] tile through LDS: rows of 256 bytes in, and out 16 bytes per
//                lane with ck / 8 adjacent lanes on one row's 128-byte K-step (hi | lo of the interleaved layout included).  The
//                per-channel maximum of the IEEE-half modes is a column reduction with the lanes along Cout, split over row
//                ranges into partial maxima the pack blocks finish (a maximum is exact in any order).  The rotated kernel of the
//                data gradient keeps 32 output channels contiguous: a gather copy, one thread per output float.
//                The first layer (Cin = 3 in a 4-channel slot, 27 weights per channel) has a small kernel of its own.
//                The IRNet heads and the plain stacks come through the same jobs, the heads at k = 1: a job without a bias
//                (b_off < 0) gets b1 = 0, and one whose input is wider than its tensor (Cin_pad: the final edge conv, 160 in 192)
//                packs zeros for the channels past Cin; a DeepLab job has neither.
//                Four launches for the whole net, whatever its depth: each kernel finds its layer in a device table of per-layer
//                jobs built once per gradient object (a launch per layer and kernel was launch-bound: ~10 us each, 75 of them).
//   vectors      GroupNorm weight / bias of every head (IRNet), BatchNorm gamma / beta and biases (01_train), copied from the
//                parameter buffer to the net's device vectors: one launch from a job table.
//   fold         BatchNorm's inference form of a conv's epilogue from the updated affine parameters and the running statistics the
//                training forward pass keeps on the device: sc = gamma / sqrt(var + eps), b = beta - mean sc in double (net.hip's
//                fold_bn, operation for operation), each rounded to float once.  One thread per channel, one launch from a job table.
//   transpose    the classifier's Linear lies as torch's [C][F]; the conv rows read [Cin][Cout] = [F][C]: a copy through one index
//                swap into the gradient object's own buffer (20 x 1024 floats: nothing to tile).
#include "common.h"

#include <algorithm>

namespace {

constexpr int REPACK_PMAX_SPLITS = 64; // row ranges of a layer's partial channel maxima, at most

// Every job-table kernel below is ONE launch over all jobs: block b belongs to the job whose block range holds it.  BLOCK0 is the
// member with the job's first block in this launch; the host half of the contract (JobTable<Job>::add of net.hip, repack_plan
// here): jobs in order, BLOCK0 non-decreasing, a job without blocks in a launch has an empty range.  Returns the job; *lb: the
// block's index inside it.
template <class Job, int Job::*BLOCK0> __device__ __forceinline__ const Job &find_job(const Job *jobs, int n_jobs, int *lb) {
    int ji = 0;
    while (ji + 1 < n_jobs && (int)blockIdx.x >= jobs[ji + 1].*BLOCK0) ++ji;
    *lb = (int)blockIdx.x - jobs[ji].*BLOCK0;
    return jobs[ji];
}

// pmax[split][c] = max |w[r][c]| over the split's rows (a NaN is passed over, as std::max passes it over in make_conv: the pack
// kernels below raise the range flag for it);
// block (tile, split) of a layer = lb % tiles, lb / tiles
__global__ __launch_bounds__(256) void repack_colmax_kernel(const RepackJob *__restrict__ jobs, int n_jobs, const float *__restrict__ param,
                                                            float *__restrict__ pmax_all) {
    __shared__ float red[4][64];
    int lb;
    const RepackJob &J = find_job<RepackJob, &RepackJob::max_block0>(jobs, n_jobs, &lb);
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
    int lb;
    const RepackJob &J = find_job<RepackJob, &RepackJob::pack_block0>(jobs, n_jobs, &lb);
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
    int lb;
    const RepackJob &J = find_job<RepackJob, &RepackJob::rot_block0>(jobs, n_jobs, &lb);
    const RepackJob *next = &J + 1; // the layer's blocks end where the next layer's begin
    const int nb = (next < jobs + n_jobs ? next->rot_block0 : (int)gridDim.x) - J.rot_block0;
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

// block lb of a job copies its floats [VEC_COPY_PER_BLOCK lb, ...)
__global__ __launch_bounds__(VEC_COPY_PER_BLOCK) void vec_copy_kernel(const VecCopyJob *__restrict__ jobs, int n_jobs,
                                                                      const float *__restrict__ param, unsigned *range) {
    int lb;
    const VecCopyJob &J = find_job<VecCopyJob, &VecCopyJob::block0>(jobs, n_jobs, &lb);
    const int i = lb * VEC_COPY_PER_BLOCK + threadIdx.x;
    if (i < J.n) {
        const float v = param[J.off + i];
        J.dst[i] = v;
        if (!(fabsf(v) < INFINITY)) *range = (unsigned)J.n; // (a non-finite parameter: the door of the range guard, as the conv rows')
    }
}

// block lb of a job folds its channels [BN_FOLD_PER_BLOCK lb, ...)
__global__ __launch_bounds__(BN_FOLD_PER_BLOCK) void bn_fold_kernel(const BnFoldJob *__restrict__ jobs, int n_jobs, const float *__restrict__ param,
                                                                    const float *__restrict__ run, unsigned *range) {
    int lb;
    const BnFoldJob &J = find_job<BnFoldJob, &BnFoldJob::block0>(jobs, n_jobs, &lb);
    const int c = lb * BN_FOLD_PER_BLOCK + threadIdx.x;
    if (c >= J.C) return;
    const double gamma = (double)param[J.g_off + c], beta = (double)param[J.be_off + c];
    const double mean = (double)run[J.run_off + c], var = (double)run[J.run_off + J.C + c];
    const double sc = __ddiv_rn(gamma, __dsqrt_rn(__dadd_rn(var, J.eps)));
    const float s = __double2float_rn(sc), b = __double2float_rn(__dsub_rn(beta, __dmul_rn(mean, sc)));
    J.s2[c] = s;
    J.b2[c] = b;
    // (a scale / shift that is not finite: the door of the range guard, as make_conv's for what the host folds)
    if (!(fabsf(s) < INFINITY) || !(fabsf(b) < INFINITY)) *range = (unsigned)J.C;
}

// dst[f][c] = src[c][f]: one thread per float of dst
__global__ __launch_bounds__(256) void transpose_cf_kernel(const float *__restrict__ src, int C, int F, float *__restrict__ dst) {
    const int total = C * F;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        const int f = o / C, c = o - f * C;
        dst[o] = src[(long long)c * F + f];
    }
}

} // namespace

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
                int splits = std::max(1, std::min(std::min(512 / J.tiles, REPACK_PMAX_SPLITS), (R + 15) / 16));
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

int vec_copy_launch(wsc_ctx *ctx, const VecCopyJob *jobs_dev, int n_jobs, int blocks, const float *param) {
    if (n_jobs <= 0 || blocks <= 0) return WSC_OK;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 8.0 * blocks * VEC_COPY_PER_BLOCK);
    hipLaunchKernelGGL(vec_copy_kernel, dim3(blocks), dim3(VEC_COPY_PER_BLOCK), 0, ctx->stream, jobs_dev, n_jobs, param, ctx->range_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int bn_fold_launch(wsc_ctx *ctx, const BnFoldJob *jobs_dev, int n_jobs, int blocks, const float *param, const float *run) {
    if (n_jobs <= 0 || blocks <= 0) return WSC_OK;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 24.0 * blocks * BN_FOLD_PER_BLOCK);
    hipLaunchKernelGGL(bn_fold_kernel, dim3(blocks), dim3(BN_FOLD_PER_BLOCK), 0, ctx->stream, jobs_dev, n_jobs, param, run, ctx->range_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int transpose_cf_launch(wsc_ctx *ctx, const float *src, int C, int F, float *dst) {
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 8.0 * C * F);
    hipLaunchKernelGGL(transpose_cf_kernel, dim3(wsc_grid_for((long long)C * F)), dim3(256), 0, ctx->stream, src, C, F, dst);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}
