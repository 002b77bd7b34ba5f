// cls_sgd.hip -- the update half of a 01_train step (Keras 2.2 optimizers.SGD(lr, momentum, decay=0.0, nesterov).get_updates,
// 01_train/demo.py:60) on the flat fp32 layout of wsc_cls_param_layout, and the two kernels the repack of the plain stacks needs on
// top of seg_sgd.hip's / irn_sgd.hip's: wsc_cls_sgd_step and wsc_net_cls_load_params of net.hip.  Built with -ffp-contract=off, and
// every product, sum, quotient and root below is spelled with its round-to-nearest intrinsic: one rounding each.
//
//   step         v = momentum m - lr g;  m = v;  p = (p + momentum v) - lr g (nesterov) or p + v.  lr g is formed ONCE and used
//                twice.  One rate for every parameter, no weight decay, so an element needs nothing but its own three floats: one
//                thread per 16-byte vector, three streams in, two out.  A buffer off the 16-byte grid takes the scalar form, the same
//                expressions per element.
//   fold         BatchNorm's inference form of a conv's epilogue from the updated affine parameters and the running statistics the
//                training forward pass keeps on the device: sc = gamma / sqrt(var + eps), b = beta - mean sc in double (net.hip's
//                fold_bn, operation for operation), each rounded to float once.  One thread per channel, one launch from a job table.
//   transpose    the classifier's Linear lies as torch's [C][F]; the repack reads [Cin][Cout] = [F][C]: a copy through one index swap
//                into the gradient object's own buffer (20 x 1024 floats: nothing to tile).
#include "common.h"

#include <algorithm>

namespace {

constexpr int CSGD_BLOCK = 256;

template <bool NESTEROV>
__device__ __forceinline__ void cls_sgd_one(float &p, float g, float &m, float lr, float mo) {
    const float lg = __fmul_rn(lr, g);
    const float v = __fsub_rn(__fmul_rn(mo, m), lg);
    m = v;
    p = NESTEROV ? __fsub_rn(__fadd_rn(p, __fmul_rn(mo, v)), lg) : __fadd_rn(p, v);
}

template <bool VEC, bool NESTEROV>
__global__ __launch_bounds__(CSGD_BLOCK) void cls_sgd_kernel(float *param, const float *grad, float *mom, long long elems, float lr, float mo) {
    constexpr int PER = VEC ? 4 : 1;
    const long long nvec = (elems + PER - 1) / PER;
    for (long long v = (long long)blockIdx.x * CSGD_BLOCK + threadIdx.x; v < nvec; v += (long long)gridDim.x * CSGD_BLOCK) {
        const long long base = v * PER;
        if (VEC && base + 4 <= elems) {
            const float4 p4 = *reinterpret_cast<const float4 *>(param + base);
            const float4 g4 = *reinterpret_cast<const float4 *>(grad + base);
            const float4 m4 = *reinterpret_cast<const float4 *>(mom + base);
            float p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
            const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) cls_sgd_one<NESTEROV>(p[e], g[e], m[e], lr, mo);
            *reinterpret_cast<float4 *>(mom + base) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(param + base) = make_float4(p[0], p[1], p[2], p[3]);
        } else {
            for (long long i = base; i < base + PER && i < elems; ++i) {
                float p = param[i], m = mom[i];
                cls_sgd_one<NESTEROV>(p, grad[i], m, lr, mo);
                mom[i] = m;
                param[i] = p;
            }
        }
    }
}

// block b folds channels [BN_FOLD_PER_BLOCK lb, ...) of the job whose block range holds it
__global__ __launch_bounds__(BN_FOLD_PER_BLOCK) void bn_fold_kernel(const BnFoldJob *__restrict__ jobs, int n_jobs, const float *__restrict__ param,
                                                                    const float *__restrict__ run, unsigned *range) {
    int ji = 0;
    while (ji + 1 < n_jobs && (int)blockIdx.x >= jobs[ji + 1].block0) ++ji;
    const BnFoldJob &J = jobs[ji];
    const int c = ((int)blockIdx.x - J.block0) * BN_FOLD_PER_BLOCK + threadIdx.x;
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

int cls_sgd_launch(wsc_ctx *ctx, float *param, const float *grad, float *mom, long long elems, float lr, float momentum, int nesterov) {
    const bool vec = aligned16(param) && aligned16(grad) && aligned16(mom);
    const long long nvec = vec ? (elems + 3) / 4 : elems;
    const dim3 grid((unsigned)std::min<long long>(std::max<long long>((nvec + CSGD_BLOCK - 1) / CSGD_BLOCK, 1), 8192)), block(CSGD_BLOCK);
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 20.0 * elems);
    if (vec && nesterov) hipLaunchKernelGGL((cls_sgd_kernel<true, true>), grid, block, 0, ctx->stream, param, grad, mom, elems, lr, momentum);
    else if (vec) hipLaunchKernelGGL((cls_sgd_kernel<true, false>), grid, block, 0, ctx->stream, param, grad, mom, elems, lr, momentum);
    else if (nesterov) hipLaunchKernelGGL((cls_sgd_kernel<false, true>), grid, block, 0, ctx->stream, param, grad, mom, elems, lr, momentum);
    else hipLaunchKernelGGL((cls_sgd_kernel<false, false>), grid, block, 0, ctx->stream, param, grad, mom, elems, lr, momentum);
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
