// irn_sgd.hip -- the update half of an IRNet training step (step/train_irn.py:86-90, 127-129) on the flat fp32 layout of
// wsc_irn_grad_layout, the vectors of the repack that brings the updated floats into a net, and the per-channel mean of the closing
// dp_mean pass (train_irn.py:148-164): wsc_irn_sgd_step, wsc_net_irn_load_params and wsc_channel_mean_nchw of net.hip.  Built
// with -ffp-contract=off: every product and sum below is one fp32 rounding, spelled with __fmul_rn / __fadd_rn / __fsub_rn.
//
//   step         torch.optim.SGD with dampening 0, no Nesterov: g = grad + wd p; m = momentum m + g; p = p - lr m, three streams in,
//                two out.  The layout has the edge group first and the dp group behind it, so ONE offset tells an element's
//                learning rate: a comparison per element, no table.  The boundary is any (the edge conv's one-float bias makes it
//                odd), so a 16-byte vector may straddle it; a buffer that is not 16-byte aligned takes the scalar form, the
//                same expressions per element.
//   vectors      GroupNorm weight / bias of every head, copied from the parameter buffer to the head's device vectors: one launch
//                from a job table (the conv weights go through seg_sgd.hip's repack, the edge conv's bias through its b1).
//   channel mean x [N][C][HW] -> mean[c] over (n, p) in double: block (b, c) sums the items b 256 + t + k B 256 of channel c, each
//                thread in ascending k, the block in block_sum's order; partial[c][b] to HBM; the block of a channel that arrives
//                last (an integer ticket per channel, agent-scope release / acquire) adds the partials in block order, divides
//                by N HW and subtracts sub[c].  No floating-point atomic: two calls give the same bits.  An item is four
//                consecutive floats of one plane (added in order) where HW % 4 == 0 and x is 16-byte aligned, else one float.
#include "common.h"

#include <algorithm>

namespace {

constexpr int ISGD_BLOCK = 256;

__device__ __forceinline__ void irn_sgd_one(float &p, float g, float &m, float lr, float wd, float mo) {
    const float t = __fadd_rn(g, __fmul_rn(wd, p));
    m = __fadd_rn(__fmul_rn(mo, m), t);
    p = __fsub_rn(p, __fmul_rn(lr, m));
}

template <bool VEC>
__global__ __launch_bounds__(ISGD_BLOCK) void irn_sgd_kernel(float *param, const float *grad, float *mom, long long elems, long long boundary,
                                                             float lr_a, float lr_b, float wd, float mo) {
    constexpr int PER = VEC ? 4 : 1;
    const long long nvec = (elems + PER - 1) / PER;
    for (long long v = (long long)blockIdx.x * ISGD_BLOCK + threadIdx.x; v < nvec; v += (long long)gridDim.x * ISGD_BLOCK) {
        const long long base = v * PER;
        if (VEC && base + 4 <= elems) {
            const float4 p4 = *reinterpret_cast<const float4 *>(param + base);
            const float4 g4 = *reinterpret_cast<const float4 *>(grad + base);
            const float4 m4 = *reinterpret_cast<const float4 *>(mom + base);
            float p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
            const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) irn_sgd_one(p[e], g[e], m[e], base + e < boundary ? lr_a : lr_b, wd, mo);
            *reinterpret_cast<float4 *>(mom + base) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(param + base) = make_float4(p[0], p[1], p[2], p[3]);
        } else {
            for (long long i = base; i < base + PER && i < elems; ++i) {
                float p = param[i], m = mom[i];
                irn_sgd_one(p, grad[i], m, i < boundary ? lr_a : lr_b, wd, mo);
                mom[i] = m;
                param[i] = p;
            }
        }
    }
}

// block b copies floats [VEC_COPY_PER_BLOCK lb, ...) of the job whose block range holds it
__global__ __launch_bounds__(VEC_COPY_PER_BLOCK) void vec_copy_kernel(const VecCopyJob *__restrict__ jobs, int n_jobs,
                                                                      const float *__restrict__ param, unsigned *range) {
    int ji = 0;
    while (ji + 1 < n_jobs && (int)blockIdx.x >= jobs[ji + 1].block0) ++ji;
    const VecCopyJob &J = jobs[ji];
    const int i = ((int)blockIdx.x - J.block0) * VEC_COPY_PER_BLOCK + threadIdx.x;
    if (i < J.n) {
        const float v = param[J.off + i];
        J.dst[i] = v;
        if (!(fabsf(v) < INFINITY)) *range = (unsigned)J.n; // (a non-finite parameter: the door of the range guard, as the repack's)
    }
}

struct ChannelMeanArgs {
    const float *x;
    long long HW, count; // count = N HW
    int C;
    const float *sub; // or null
    double *partials; // [C][gridDim.x]
    unsigned *tickets; // [C], zero at launch
    double *out;
};

template <bool VEC>
__global__ __launch_bounds__(ISGD_BLOCK) void channel_mean_kernel(ChannelMeanArgs a) {
    __shared__ double scratch[ISGD_BLOCK / 64], fin[CHANNEL_MEAN_MAX_BLOCKS];
    __shared__ int s_last;
    const int tid = threadIdx.x, c = blockIdx.y;
    constexpr int PER = VEC ? 4 : 1;
    const long long items = a.count / PER, per_plane = a.HW / PER; // (VEC: HW % 4 == 0)
    double s[1] = {0.0};
    for (long long i = (long long)blockIdx.x * ISGD_BLOCK + tid; i < items; i += (long long)gridDim.x * ISGD_BLOCK) {
        const long long n = i / per_plane, q = i - n * per_plane;
        const float *src = a.x + (n * a.C + c) * a.HW + q * PER;
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4 *>(src);
            s[0] += (((double)v.x + (double)v.y) + (double)v.z) + (double)v.w;
        } else {
            s[0] += (double)*src;
        }
    }
    block_sum<1>(s, scratch);
    if (tid == 0) {
        a.partials[(long long)c * gridDim.x + blockIdx.x] = s[0];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(a.tickets + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == gridDim.x - 1;
        if (s_last) { // every block's partial of this channel is out
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    for (unsigned b = tid; b < gridDim.x; b += ISGD_BLOCK) fin[b] = a.partials[(long long)c * gridDim.x + b];
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) t += fin[b];
        t /= (double)a.count;
        if (a.sub) t -= (double)a.sub[c];
        a.out[c] = t;
    }
}

} // namespace

int irn_sgd_launch(wsc_ctx *ctx, float *param, const float *grad, float *mom, long long elems, long long boundary, float lr_a, float lr_b,
                   float weight_decay, float momentum) {
    const bool vec = aligned16(param) && aligned16(grad) && aligned16(mom);
    const long long nvec = vec ? (elems + 3) / 4 : elems;
    const int blocks = (int)std::min<long long>(std::max<long long>((nvec + ISGD_BLOCK - 1) / ISGD_BLOCK, 1), 8192);
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 20.0 * elems);
    if (vec)
        hipLaunchKernelGGL(irn_sgd_kernel<true>, dim3(blocks), dim3(ISGD_BLOCK), 0, ctx->stream, param, grad, mom, elems, boundary, lr_a, lr_b,
                           weight_decay, momentum);
    else
        hipLaunchKernelGGL(irn_sgd_kernel<false>, dim3(blocks), dim3(ISGD_BLOCK), 0, ctx->stream, param, grad, mom, elems, boundary, lr_a, lr_b,
                           weight_decay, momentum);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int vec_copy_launch(wsc_ctx *ctx, const VecCopyJob *jobs_dev, int n_jobs, int blocks, const float *param) {
    if (n_jobs <= 0 || blocks <= 0) return WSC_OK;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 8.0 * blocks * VEC_COPY_PER_BLOCK);
    hipLaunchKernelGGL(vec_copy_kernel, dim3(blocks), dim3(VEC_COPY_PER_BLOCK), 0, ctx->stream, jobs_dev, n_jobs, param, ctx->range_dev);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int channel_mean_launch(wsc_ctx *ctx, const float *x, int N, int C, long long HW, const float *sub_host, double *out) {
    WSC_CHECK(N > 0 && C > 0 && C <= CHANNEL_MEAN_MAX_C && HW > 0, WSC_ERR_INVALID, "channel mean: %d x %d x %lld", N, C, HW);
    const bool vec = HW % 4 == 0 && aligned16(x);
    const long long count = (long long)N * HW, items = vec ? count / 4 : count;
    const int blocks = (int)std::min<long long>(std::max<long long>((items + 4 * ISGD_BLOCK - 1) / (4 * ISGD_BLOCK), 1), CHANNEL_MEAN_MAX_BLOCKS);
    // one block of scratch: the tickets, the subtrahend, the partials
    const size_t vec_b = ((size_t)C * 4 + 255) / 256 * 256;
    void *blk = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, 2 * vec_b + sizeof(double) * (size_t)C * blocks, &blk));
    WscCachedGuard guard(ctx, blk);
    ChannelMeanArgs a;
    a.x = x; a.HW = HW; a.count = count; a.C = C;
    a.tickets = (unsigned *)blk;
    a.sub = sub_host ? (const float *)((char *)blk + vec_b) : nullptr;
    a.partials = (double *)((char *)blk + 2 * vec_b);
    a.out = out;
    WSC_HIP(hipMemsetAsync(a.tickets, 0, vec_b, ctx->stream)); // (the tickets start at zero whatever the block held)
    if (sub_host) WSC_TRY(wsc_ctx_upload_small(ctx, (char *)blk + vec_b, sub_host, sizeof(float) * C));
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 4.0 * count * C);
    if (vec) hipLaunchKernelGGL(channel_mean_kernel<true>, dim3(blocks, C), dim3(ISGD_BLOCK), 0, ctx->stream, a);
    else hipLaunchKernelGGL(channel_mean_kernel<false>, dim3(blocks, C), dim3(ISGD_BLOCK), 0, ctx->stream, a);
    WSC_HIP(hipGetLastError());
    guard.free_now();
    return WSC_OK;
}
