// seg_dropout.hip -- the dropout sites of the SEC / DSRG training graph (drop6 / drop7, SEC.py:123,225-227; drop6_k / drop7_k,
// DSRG.py:174-177,276-278) on the activations fc6 / fc7 left, with the project's own counter-based keep-masks (DESIGN.md section 7:
// TensorFlow's random stream is not reproduced).  Built with -ffp-contract=off: every product below is one fp32 rounding.
//
//   mask      Philox4x32-10, key = (seed low, seed high), counter = (low(i >> 2), high(i >> 2), step, site) for element i of the
//             [B][h][w][Cout] tensor; element i takes output word i & 3.  u = float(word >> 8) 2^-24 (exact), keep iff u >= drop_prob.
//             A mask depends on (seed, step, site, i) alone: not on the launch geometry, the precision or the vector width.
//   value     d = y scale on kept elements, +0.0 on dropped ones, scale = 1 / (1 - drop_prob) in fp32; y = hi + lo of a two-plane
//             activation.  d is stored by the split of the conv epilogue's generic path (hi = half(d) saturating, lo = half(clamp(d) -
//             hi)); a stored IEEE half at the ceiling raises the ctx's range flag as a conv epilogue does.
//   tape      optional: the fp32 value the planes now hold (what the next op reads), written in the same pass -- in place of the
//             launch_act_to_f32 copy behind fc6 / fc7.
//   form      one thread per 16 bytes of a plane: 4 fp32 or 8 16-bit elements, i.e. one or two Philox blocks.  The loads are issued
//             first and the ten rounds (20 32 x 32 -> 64 multiplies a block, not full rate) run under their latency; nothing of a
//             round depends on a loaded value.  A tensor whose first element is off the 4-element grid of the counter, or a buffer
//             off the 16-byte grid, takes the scalar form: one element and one block per thread, the same words.
#include "common.h"
#include "dropout_rng.h" // (Philox4x32-10, DropRng, the keep rule and the value: one definition of the counter layout)

namespace {

constexpr int DROP_BLOCK = 256; // four waves of 64

// fp32: y[i] = dropout of x[i] (y may be x), element i has index first + i; keep / tape: optional.  VEC: first % 4 == 0 and every
// buffer on its vector grid (16 bytes; 4 for keep).
template <bool VEC>
__global__ __launch_bounds__(DROP_BLOCK) void dropout_f32_kernel(const float *x, float *y, float *tape, uint8_t *keep, long long n,
                                                                  unsigned long long first, DropRng g) {
    const long long t = (long long)blockIdx.x * DROP_BLOCK + threadIdx.x;
    uint32_t w[4];
    if (!VEC) {
        if (t >= n) return;
        const float v = x[t];
        const unsigned long long gi = first + (unsigned long long)t;
        drop_words(g, gi >> 2, w);
        const bool k = drop_keeps(g, w[gi & 3]);
        const float d = drop_value(g, v, k);
        y[t] = d;
        if (tape) tape[t] = d;
        if (keep) keep[t] = k ? 1 : 0;
        return;
    }
    const long long base = 4 * t;
    if (base >= n) return;
    const bool full = base + 4 <= n;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (full) {
        const float4 v4 = *reinterpret_cast<const float4 *>(x + base);
        v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
    } else {
        for (int e = 0; base + e < n; ++e) v[e] = x[base + e];
    }
    drop_words(g, (first >> 2) + (unsigned long long)t, w);
    float d[4];
    uint32_t kb = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool k = drop_keeps(g, w[e]);
        d[e] = drop_value(g, v[e], k);
        kb |= (k ? 1u : 0u) << (8 * e);
    }
    if (full) {
        const float4 d4 = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<float4 *>(y + base) = d4;
        if (tape) *reinterpret_cast<float4 *>(tape + base) = d4;
        if (keep) *reinterpret_cast<uint32_t *>(keep + base) = kb;
    } else {
        for (int e = 0; base + e < n; ++e) {
            y[base + e] = d[e];
            if (tape) tape[base + e] = d[e];
            if (keep) keep[base + e] = (uint8_t)((kb >> (8 * e)) & 1u);
        }
    }
}

// one element of the 16-bit planes: the stored halves, the fp32 value they hold, whether the hi half is at the IEEE ceiling
__device__ __forceinline__ void drop_store_h16(float d, int fmt, bool split, uint16_t *h, uint16_t *l, float *held, bool *ceil) {
    const uint16_t hh = f32_to_h16(d, fmt);
    float r = h16_to_f32(hh, fmt);
    uint16_t ll = 0;
    if (split) {
        // (the generic conv epilogue's: the lo plane has the hi plane's format; a value beyond half's range saturates as a whole)
        const float c = fmt ? fminf(fmaxf(d, -65504.f), 65504.f) : d;
        ll = f32_to_h16(__fsub_rn(c, r), fmt);
        r = __fadd_rn(r, h16_to_f32(ll, fmt));
    }
    *h = hh; *l = ll; *held = r;
    *ceil = fmt == 1 && (hh & 0x7fffu) >= 0x7bffu;
}
__device__ __forceinline__ float drop_load_h16(uint16_t h, uint16_t l, int fmt, bool split) {
    float v = h16_to_f32(h, fmt);
    if (split) v = __fadd_rn(v, h16_to_f32(l, fmt));
    return v;
}

// the 16-bit planes in place (lo null: one plane), the tensor's first element at index 0.  VEC: 8 elements = 16 bytes of a plane
// and two counter blocks per thread.
template <bool VEC>
__global__ __launch_bounds__(DROP_BLOCK) void dropout_h16_kernel(uint16_t *hi, uint16_t *lo, float *tape, long long n, int fmt, DropRng g,
                                                                  unsigned *range, unsigned range_mark) {
    const long long t = (long long)blockIdx.x * DROP_BLOCK + threadIdx.x;
    const bool split = lo != nullptr;
    bool ovf = false;
    if (!VEC) {
        if (t < n) {
            const float v = drop_load_h16(hi[t], split ? lo[t] : (uint16_t)0, fmt, split);
            uint32_t w[4];
            drop_words(g, (unsigned long long)t >> 2, w);
            uint16_t h, l;
            float held;
            drop_store_h16(drop_value(g, v, drop_keeps(g, w[t & 3])), fmt, split, &h, &l, &held, &ovf);
            hi[t] = h;
            if (split) lo[t] = l;
            if (tape) tape[t] = held;
        }
    } else if (8 * t < n) {
        const long long base = 8 * t;
        const bool full = base + 8 <= n;
        uint16_t hv[8] = {}, lv[8] = {};
        if (full) {
            const uint4 h4 = *reinterpret_cast<const uint4 *>(hi + base);
            const uint32_t hw[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { hv[2 * j] = (uint16_t)(hw[j] & 0xffffu); hv[2 * j + 1] = (uint16_t)(hw[j] >> 16); }
            if (split) {
                const uint4 l4 = *reinterpret_cast<const uint4 *>(lo + base);
                const uint32_t lw[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) { lv[2 * j] = (uint16_t)(lw[j] & 0xffffu); lv[2 * j + 1] = (uint16_t)(lw[j] >> 16); }
            }
        } else {
            for (int e = 0; base + e < n; ++e) {
                hv[e] = hi[base + e];
                if (split) lv[e] = lo[base + e];
            }
        }
        uint32_t w[8];
        drop_words(g, 2ull * (unsigned long long)t, w);
        drop_words(g, 2ull * (unsigned long long)t + 1, w + 4);
        uint16_t ho[8], lw_o[8];
        float held[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = drop_load_h16(hv[e], lv[e], fmt, split);
            bool c;
            drop_store_h16(drop_value(g, v, drop_keeps(g, w[e])), fmt, split, &ho[e], &lw_o[e], &held[e], &c);
            if (full || base + e < n) ovf |= c;
        }
        if (full) {
            auto pk = [](uint16_t a, uint16_t b) { return (uint32_t)a | ((uint32_t)b << 16); };
            *reinterpret_cast<uint4 *>(hi + base) = make_uint4(pk(ho[0], ho[1]), pk(ho[2], ho[3]), pk(ho[4], ho[5]), pk(ho[6], ho[7]));
            if (split)
                *reinterpret_cast<uint4 *>(lo + base) = make_uint4(pk(lw_o[0], lw_o[1]), pk(lw_o[2], lw_o[3]), pk(lw_o[4], lw_o[5]), pk(lw_o[6], lw_o[7]));
            if (tape) {
                *reinterpret_cast<float4 *>(tape + base) = make_float4(held[0], held[1], held[2], held[3]);
                *reinterpret_cast<float4 *>(tape + base + 4) = make_float4(held[4], held[5], held[6], held[7]);
            }
        } else {
            for (int e = 0; base + e < n; ++e) {
                hi[base + e] = ho[e];
                if (split) lo[base + e] = lw_o[e];
                if (tape) tape[base + e] = held[e];
            }
        }
    }
    if (ovf) *range = range_mark; // (a plain store of a non-zero value: every writer writes "raised")
}

bool aligned_to(const void *p, unsigned a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }

int drop_grid(long long n, int per, unsigned *blocks) {
    const long long b = ((n + per - 1) / per + DROP_BLOCK - 1) / DROP_BLOCK;
    WSC_CHECK(b >= 1 && b < (1ll << 31), WSC_ERR_INVALID, "dropout: %lld elements", n);
    *blocks = (unsigned)b;
    return WSC_OK;
}

} // namespace

int seg_dropout_check(const char *fn, float drop_prob, long long step) {
    WSC_CHECK(drop_prob >= 0.f && drop_prob < 1.f, WSC_ERR_INVALID, "%s: drop_prob=%g is not in [0, 1)", fn, (double)drop_prob); // (NaN fails both)
    WSC_CHECK(step >= 0 && step < (1ll << 32), WSC_ERR_INVALID, "%s: step=%lld is not in [0, 2^32)", fn, step);
    return WSC_OK;
}

float seg_dropout_scale(float drop_prob) { return 1.0f / (1.0f - drop_prob); }

int launch_seg_dropout_f32(wsc_ctx *ctx, const float *x, float *y, float *tape, uint8_t *keep, long long n, unsigned long long first,
                           float drop_prob, unsigned long long seed, unsigned step, unsigned site) {
    const DropRng g = drop_rng(drop_prob, seed, step, site);
    const bool vec = (first & 3ull) == 0 && aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(tape, 16) && aligned_to(keep, 4);
    unsigned blocks;
    WSC_TRY(drop_grid(n, vec ? 4 : 1, &blocks));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)n * (8 + (tape ? 4 : 0) + (keep ? 1 : 0)));
    if (vec) hipLaunchKernelGGL(dropout_f32_kernel<true>, dim3(blocks), dim3(DROP_BLOCK), 0, ctx->stream, x, y, tape, keep, n, first, g);
    else hipLaunchKernelGGL(dropout_f32_kernel<false>, dim3(blocks), dim3(DROP_BLOCK), 0, ctx->stream, x, y, tape, keep, n, first, g);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_seg_dropout(wsc_ctx *ctx, Act a, size_t n, int Cout, float drop_prob, unsigned long long seed, unsigned step, unsigned site,
                       float *tape) {
    if (a.is_f32()) return launch_seg_dropout_f32(ctx, a.f32(), a.f32(), tape, nullptr, (long long)n, 0ull, drop_prob, seed, step, site);
    const DropRng g = drop_rng(drop_prob, seed, step, site);
    const bool vec = aligned_to(a.hi, 16) && aligned_to(a.lo, 16) && aligned_to(tape, 16);
    unsigned blocks;
    WSC_TRY(drop_grid((long long)n, vec ? 8 : 1, &blocks));
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)n * ((a.lo ? 8 : 4) + (tape ? 4 : 0)));
    if (vec)
        hipLaunchKernelGGL(dropout_h16_kernel<true>, dim3(blocks), dim3(DROP_BLOCK), 0, ctx->stream, a.h16(), a.h16_lo(), tape, (long long)n,
                           a.fmt(), g, ctx->range_dev, (unsigned)Cout);
    else
        hipLaunchKernelGGL(dropout_h16_kernel<false>, dim3(blocks), dim3(DROP_BLOCK), 0, ctx->stream, a.h16(), a.h16_lo(), tape, (long long)n,
                           a.fmt(), g, ctx->range_dev, (unsigned)Cout);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

extern "C" {

int wsc_seg_dropout_f32(wsc_ctx *ctx, const float *x_dev, long long elems, long long first, float drop_prob, unsigned long long seed,
                        long long step, int site, float *y_dev, unsigned char *keep_dev) {
    WSC_CHECK(ctx && x_dev && y_dev, WSC_ERR_INVALID, "wsc_seg_dropout_f32: null argument");
    WSC_CHECK(elems >= 1 && first >= 0 && first <= (1ll << 62) && site >= 0, WSC_ERR_INVALID, "wsc_seg_dropout_f32: %lld elements from %lld, site %d",
              elems, first, site);
    WSC_TRY(seg_dropout_check("wsc_seg_dropout_f32", drop_prob, step));
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_seg_dropout_f32(ctx, x_dev, y_dev, nullptr, keep_dev, elems, (unsigned long long)first, drop_prob, seed, (unsigned)step,
                                  (unsigned)site);
}

} // extern "C"
