// sgd.hip -- the update half of the three training steps, each on the flat fp32 parameter layout of its gradient object:
// wsc_seg_sgd_accumulate / wsc_seg_sgd_apply (SEC / DSRG: Model.optimize(), model.py:379-404), wsc_irn_sgd_step (IRNet:
// step/train_irn.py:86-90, 127-129) and wsc_cls_sgd_step (01_train: Keras 2.2 optimizers.SGD(lr, momentum, decay=0.0,
// nesterov).get_updates, 01_train/demo.py:60) of net.hip.  Built with -ffp-contract=off, and every product, sum and quotient below
// is spelled with its round-to-nearest intrinsic: one fp32 rounding each.
//
//   update       ONE streaming kernel for apply and the two steps: one thread per 16-byte vector of three fp32 streams (the
//                parameters, the gradient or its accumulator, the momentum), three in, two out.  A `Step` holds the scalars of an
//                optimiser and its per-element function; the element's index comes with it, so a vector may straddle a boundary
//                of the layout.  A buffer that is not 16-byte aligned takes the scalar form, the same expressions per element.
//     apply      mom = mom momentum + accum; param = param - lr mom; accum = +0.0 (clear: the one store into the middle stream)
//     irn        torch.optim.SGD with dampening 0, no Nesterov: g = grad + wd p; m = momentum m + g; p = p - lr m.  The layout has
//                the edge group first and the dp group behind it, so ONE offset tells an element's learning rate: a comparison per
//                element, no table.  The boundary is any (the edge conv's one-float bias makes it odd).
//     cls        v = momentum m - lr g;  m = v;  p = (p + momentum v) - lr g (nesterov) or p + v.  lr g is formed ONCE and used
//                twice.  One rate for every parameter, no weight decay.
//   accumulate   t = grad + wd param (weights), t = grad (biases); t = mult t; accum += t / accum_num.  One thread per 16-byte vector
//                of the WHOLE buffer: the layers' offsets are any (a 5-class fc8 bias makes every later one odd), so a vector may
//                straddle segments; an element's segment is found by bisection of the table (in LDS) for the vector's first float
//                and stepped forward per element.  The per-thread segment and the block-level tail are its own: it shares the
//                update kernel's grid formula, not its body.
//                loss["l2"] = sum w^2 / 2: per thread in double over its grid-stride elements, a fixed LDS tree per block, the
//                block partials to HBM; the block that arrives last (common.h's ticket) adds the partials in block order and
//                rounds once.  No floating-point atomic: two calls give the same bits.
#include "common.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int SGD_BLOCK = 256;
constexpr int STEP_MAX_BLOCKS = 8192; // of the irn / cls step (apply and accumulate: SGD_L2_MAX_BLOCKS)

// mom = mom momentum + accum, param -= lr mom; the middle stream is the accumulator, cleared where `clear` is set
struct ApplyStep {
    static constexpr bool CLEARS_MID = true;
    float lr, momentum;
    int clear;
    __device__ __forceinline__ void operator()(long long, float &p, float a, float &m) const {
        m = __fadd_rn(__fmul_rn(m, momentum), a);
        p = __fsub_rn(p, __fmul_rn(lr, m));
    }
};

struct IrnStep {
    static constexpr bool CLEARS_MID = false;
    long long boundary; // the first element of the dp group
    float lr_a, lr_b, wd, mo;
    __device__ __forceinline__ void operator()(long long i, float &p, float g, float &m) const {
        const float t = __fadd_rn(g, __fmul_rn(wd, p));
        m = __fadd_rn(__fmul_rn(mo, m), t);
        p = __fsub_rn(p, __fmul_rn(i < boundary ? lr_a : lr_b, m));
    }
};

template <bool NESTEROV> struct ClsStep {
    static constexpr bool CLEARS_MID = false;
    float lr, mo;
    __device__ __forceinline__ void operator()(long long, float &p, float g, float &m) const {
        const float lg = __fmul_rn(lr, g);
        const float v = __fsub_rn(__fmul_rn(mo, m), lg);
        m = v;
        p = NESTEROV ? __fsub_rn(__fadd_rn(p, __fmul_rn(mo, v)), lg) : __fadd_rn(p, v);
    }
};

// the middle stream of a step: read-only unless the step clears it
template <class Step> using StepMid = std::conditional_t<Step::CLEARS_MID, float, const float>;

template <bool VEC, class Step>
__global__ __launch_bounds__(SGD_BLOCK) void update_kernel(float *param, StepMid<Step> *mid, float *mom, long long elems, Step step) {
    constexpr int PER = VEC ? 4 : 1;
    const long long nvec = (elems + PER - 1) / PER;
    for (long long v = (long long)blockIdx.x * SGD_BLOCK + threadIdx.x; v < nvec; v += (long long)gridDim.x * SGD_BLOCK) {
        const long long base = v * PER;
        if (VEC && base + 4 <= elems) {
            const float4 p4 = *reinterpret_cast<const float4 *>(param + base);
            const float4 x4 = *reinterpret_cast<const float4 *>(mid + base);
            const float4 m4 = *reinterpret_cast<const float4 *>(mom + base);
            float p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
            const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) step(base + e, p[e], x[e], m[e]);
            *reinterpret_cast<float4 *>(mom + base) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(param + base) = make_float4(p[0], p[1], p[2], p[3]);
            if constexpr (Step::CLEARS_MID)
                if (step.clear) *reinterpret_cast<float4 *>(mid + base) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (long long i = base; i < base + PER && i < elems; ++i) {
                float p = param[i], m = mom[i];
                step(i, p, mid[i], m);
                mom[i] = m;
                param[i] = p;
                if constexpr (Step::CLEARS_MID)
                    if (step.clear) mid[i] = 0.f;
            }
        }
    }
}

// one block per SGD_BLOCK vectors (floats in the scalar form), at least one, at most max_blocks: the loops are grid-stride
int sgd_blocks(long long elems, bool vec, int max_blocks) {
    const long long nvec = vec ? (elems + 3) / 4 : elems;
    return (int)std::min<long long>(std::max<long long>((nvec + SGD_BLOCK - 1) / SGD_BLOCK, 1), max_blocks);
}

template <class Step>
int update_launch(wsc_ctx *ctx, float *param, StepMid<Step> *mid, float *mom, long long elems, int max_blocks, const Step &step) {
    const bool vec = aligned16(param) && aligned16(mid) && aligned16(mom);
    const dim3 grid(sgd_blocks(elems, vec, max_blocks)), block(SGD_BLOCK);
    if (vec) hipLaunchKernelGGL((update_kernel<true, Step>), grid, block, 0, ctx->stream, param, mid, mom, elems, step);
    else hipLaunchKernelGGL((update_kernel<false, Step>), grid, block, 0, ctx->stream, param, mid, mom, elems, step);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

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
        ticket_publish();
        s_last = ticket_is_last(a.counter, gridDim.x);
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
    const dim3 grid(sgd_blocks(elems, vec, SGD_L2_MAX_BLOCKS)), block(SGD_BLOCK); // (the l2 bits depend on the block count)
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 16.0 * elems);
    if (l2_dev) WSC_HIP(hipMemsetAsync(l2_counter, 0, sizeof(unsigned), ctx->stream)); // (the ticket starts at zero whatever came before)
    if (vec) hipLaunchKernelGGL(sgd_accumulate_kernel<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(sgd_accumulate_kernel<false>, grid, block, 0, ctx->stream, a);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int sgd_apply_launch(wsc_ctx *ctx, float *param, float *accum, float *mom, long long elems, float lr, float momentum, int clear_accum) {
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (clear_accum ? 24.0 : 20.0) * elems);
    return update_launch(ctx, param, accum, mom, elems, SGD_L2_MAX_BLOCKS, ApplyStep{lr, momentum, clear_accum});
}

int irn_sgd_launch(wsc_ctx *ctx, float *param, const float *grad, float *mom, long long elems, long long boundary, float lr_a, float lr_b,
                   float weight_decay, float momentum) {
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 20.0 * elems);
    return update_launch(ctx, param, grad, mom, elems, STEP_MAX_BLOCKS, IrnStep{boundary, lr_a, lr_b, weight_decay, momentum});
}

int cls_sgd_launch(wsc_ctx *ctx, float *param, const float *grad, float *mom, long long elems, float lr, float momentum, int nesterov) {
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, 20.0 * elems);
    if (nesterov) return update_launch(ctx, param, grad, mom, elems, STEP_MAX_BLOCKS, ClsStep<true>{lr, momentum});
    return update_launch(ctx, param, grad, mom, elems, STEP_MAX_BLOCKS, ClsStep<false>{lr, momentum});
}
