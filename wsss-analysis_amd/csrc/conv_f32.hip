// conv_f32.hip -- the implicit-GEMM convolution of WSC_PREC_F32: fp32 weights, fp32 NHWC activations (one plane), fp32
// accumulation on v_mfma_f32_32x32x2_f32 -- bit for bit a k-ordered fmaf chain per output element, in a FIXED order (no atomics,
// no split-K): a result depends on its own pixel's inputs only, whatever the batch or the tile it lands in.
//
// Same GEMM view, K order (ConvKLayout, common.h) and epilogue order (acc * s1 + b1, residual, ReLU, post-ReLU affine) as
// conv_igemm.hip; conv_igemm_launch sends the mode's layers here.  No range guard: fp32 has the reference's range.
//
// Tile 128 x BN x 32 (BN = 128, or 64 for <= 64 output channels), four waves 2 x 2, 64 x BN/2 per wave (64 accumulators per lane
// at BN = 128), two LDS buffers, one barrier per K-step, one K-step ahead.  A K-step is 32 fp32 = one 128-byte LDS row per pixel /
// output channel: the row size, 16-byte-slot XOR swizzle and staging ownership of conv_igemm.hip's tiles.
//   generic layers (Cin % 32 == 0): a K-step = one tap of a 32-channel chunk, staged by global_load_lds_dwordx4 (swizzle on the
//       source slot, padded taps from the zero page); the tap offset is scaled by the layer's dilation.
//   small-Cin forms (NHWC4 input): a K-step = 8 pixels x 4 channels (two kernel rows of 4 pixels, or one of 8), global ->
//       register -> LDS.
// Fragments: the MFMA takes ONE fp32 per lane and operand (lane l: row l & 31, k = l >> 5).  A ds_read_b128 of slot 2 q + (l >> 5)
// gives the lane four k of its row; MFMA e of the group uses element e, so the k order inside a K-step is (q, e, l >> 5) -- a
// permutation of the chunk's channels, the same for A and B.
// Per K-step a wave issues 16 MI NI MFMAs of 64 cycles against 4 + NB DMA pieces and 4 (MI + NI) fragment reads: the kernel is
// matrix-issue-bound; it is double-buffered and otherwise untuned.
#include "common.h"

#include <type_traits>

namespace {

struct ConvF32Args {
    const float *x, *w;
    const float *s1, *b1, *s2, *b2;
    const float *res;
    float *y, *y_f32;
    int H, W, Cin, Ho, Wo, Cout;
    int ldy; // row pitch of y in elements
    int kh, kw, stride, pad, relu;
    int M, HoWo;
    unsigned div_howo_mul, div_howo_s1, div_howo_s2, div_wo_mul, div_wo_s1, div_wo_s2; // exact division, as in conv_igemm.hip
    int nk; // K-steps
    int Kw; // packed weight row length in elements
    int ntiles_n, nblocks;
    const float *zero; // >= 16 bytes of zeros in HBM: source of padded taps
    int dil;           // tap (r, s) reads input (ho * stride - pad + r * dil, wo * stride - pad + s * dil); generic layers only
};

__device__ __forceinline__ int lds_off(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ void decode_row(const ConvF32Args &p, int m, int &n, int &ho, int &wo) {
    const unsigned t1 = __umulhi(p.div_howo_mul, (unsigned)m);
    n = (int)((t1 + (((unsigned)m - t1) >> p.div_howo_s1)) >> p.div_howo_s2);
    const int rem = m - n * p.HoWo;
    const unsigned t2 = __umulhi(p.div_wo_mul, (unsigned)rem);
    ho = (int)((t2 + (((unsigned)rem - t2) >> p.div_wo_s1)) >> p.div_wo_s2);
    wo = rem - ho * p.Wo;
}

// MODE 0: generic layer, LDS-DMA staging.  MODE 1 / 2: small-Cin forms with 4 / 8 pixels per kernel row, register staging.
template <int BN, int MODE>
__global__ __launch_bounds__(256, 2) void conv_f32_kernel(ConvF32Args p) {
    constexpr bool GLDS = MODE == 0;
    constexpr int BM = 128, NT = 256, NW = 4, WC = 2;
    constexpr int WMT = 64, WN = BN / WC, MI = WMT / 32, NI = WN / 32;
    constexpr int NB = BN * 8 / NT; // B 16-byte slots per thread per K-step
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
    constexpr int CT_STRIDE = BN + 4;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6); // wave-uniform: LDS DMA destinations stay in SGPRs
    const int wm = wv / WC, wn = wv - wm * WC;

    // XCD-aware, bijective block -> tile map (consecutive tiles share the A rows)
    int tile;
    {
        const int bid = blockIdx.x;
        const int xcd = bid & 7;
        const int q = p.nblocks >> 3, r = p.nblocks & 7;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int mt = tile / p.ntiles_n;
    const int nt = tile - mt * p.ntiles_n;
    const int m0 = mt * BM;
    const int n0 = nt * BN;

    // staging ownership: conv_igemm.hip's.  DMA: wave w's i-th piece = tile rows w * 32 + i * 8 + (lane >> 3), slot position
    // lane & 7, the swizzle on the SOURCE slot.  Register path: thread t stages rows (t >> 3) + 32 i, slot t & 7.
    const int slot = t & 7;
    const int lrow = GLDS ? (wv * 32 + (lane >> 3)) : (t >> 3);
    constexpr int RSTEP = GLDS ? 8 : 32;
    int hb[4], wb[4];
    long long aoff[4]; // element offset of the row's tap (0, 0) (+ the lane's source slot on the DMA path)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = lrow + RSTEP * i;
        const int m = m0 + r;
        if (m < p.M) {
            int n, ho, wo;
            decode_row(p, m, n, ho, wo);
            hb[i] = ho * p.stride - p.pad;
            wb[i] = wo * p.stride - p.pad;
            aoff[i] = (((long long)n * p.H + hb[i]) * p.W + wb[i]) * (long long)p.Cin;
        } else {
            hb[i] = -(1 << 28); // every tap out of bounds: zeros
            wb[i] = 0;
            aoff[i] = 0;
        }
        if (GLDS) aoff[i] += (slot ^ ((r >> 1) & 7)) * 4;
    }
    const int brow0 = GLDS ? (wv * (BN / NW) + (lane >> 3)) : (t >> 3);
    const float *wrow[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int r = brow0 + RSTEP * i;
        const int ks = GLDS ? (slot ^ ((r >> 1) & 7)) : slot;
        wrow[i] = p.w + (long long)(n0 + r) * p.Kw + ks * 4;
    }

    f32x16_t acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int l31 = lane & 31;
    const int kgrp = lane >> 5;
    // the 16 MI NI MFMAs of one fragment group q: element e of every lane's four k, e = 0 .. 3
    auto mfma_group = [&](const f32x4_t(&fa)[MI], const f32x4_t(&fb)[NI]) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][e], fb[ni][e], acc[mi][ni], 0, 0, 0);
    };

    if constexpr (GLDS) {
        // The 4 + NB DMA pieces of K-step kt + 1 are issued at the top of K-step kt; the wait for them and the barrier sit at
        // its end.  Fragment reads are inline asm with their own s_waitcnt: compiler-visible ds_reads would get an
        // s_waitcnt vmcnt(0) in front (the in-flight DMA may alias them for all the compiler knows), draining the DMA before
        // the MFMAs start (conv_igemm.hip).
        int n_khi = 0, n_kwi = 0, n_cc = 0, n_kt = 0; // (tap, chunk) of the next K-step to issue: K order (chunk, kh, kw)
        auto issue = [&](int buf) __attribute__((always_inline)) {
            // (a dilated tap outside the image contributes zero like any padded tap: the bounds test below is per tap)
            const int dh = n_khi * p.dil, dw = n_kwi * p.dil;
            const long long tap = ((long long)dh * p.W + dw) * p.Cin + n_cc * 32;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hi = hb[i] + dh, wi = wb[i] + dw;
                const bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                const float *g = ok ? p.x + (aoff[i] + tap) : p.zero;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)(smem + buf * A_BYTES + wv * 4096 + i * 1024),
                                                 16, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wrow[i] + n_kt * 32),
                                                 (__attribute__((address_space(3))) void *)(smem + 2 * A_BYTES + buf * B_BYTES + wv * (NB * 1024) + i * 1024),
                                                 16, 0, 0);
            ++n_kt;
            if (++n_kwi == p.kw) {
                n_kwi = 0;
                if (++n_khi == p.kh) {
                    n_khi = 0;
                    ++n_cc;
                }
            }
        };
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
        // lds_off(row + 32 i, sl) = lds_off(row, sl) + 4096 i: one address per fragment group and operand, mi / ni and the
        // buffer in the instruction's immediate offset
        unsigned offA[4], offB[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            offA[q] = lds0 + lds_off(wm * WMT + l31, q * 2 + kgrp);
            offB[q] = lds0 + 2 * A_BYTES + lds_off(wn * WN + l31, q * 2 + kgrp);
        }
        static_assert(A_BYTES + (MI - 1) * 4096 < 65536 && B_BYTES + (NI - 1) * 4096 < 65536, "ds_read immediate offset range");
        issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        auto kstep = [&](auto cur_c, int kt) __attribute__((always_inline)) {
            constexpr int cur = decltype(cur_c)::value;
            const unsigned(&oA)[4] = offA, (&oB)[4] = offB;
            if (kt + 1 < p.nk) issue(cur ^ 1);
            f32x4_t fa[2][MI], fb[2][NI];
            auto rd = [&](int set, int q) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[set][mi]) : "v"(oA[q]), "n"(cur * A_BYTES + mi * 4096) : "memory");
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[set][ni]) : "v"(oB[q]), "n"(cur * B_BYTES + ni * 4096) : "memory");
            };
            rd(0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int set = q & 1;
                if (q < 3) {
                    rd(set ^ 1, q + 1);
                    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(MI + NI) : "memory"); // LDS returns in order: group q has landed
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                mfma_group(fa[set], fb[set]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the next K-step's pieces have landed ...
            __syncthreads();                                  // ... for every wave, and every read of this buffer is done
        };
        for (int kt = 0; kt < p.nk; kt += 2) {
            kstep(std::integral_constant<int, 0>{}, kt);
            if (kt + 1 < p.nk) kstep(std::integral_constant<int, 1>{}, kt + 1);
        }
    } else {
        // NHWC4 input: slot g of the K loop = pixel g % PPR of kernel row g / PPR (4 channels = 16 bytes), 8 slots per K-step;
        // the weights are packed to match, zero where a row has fewer than PPR columns (those pixels load zeros too)
        constexpr int PPR_LOG2 = MODE + 1;
        f32x4_t ra[4], rb[NB];
        auto load_tile = [&](int kt) __attribute__((always_inline)) {
            const int g = kt * 8 + slot;
            const int khi = g >> PPR_LOG2;
            const int px = g & ((1 << PPR_LOG2) - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hi = hb[i] + khi, wi = wb[i] + px;
                const bool ok = khi < p.kh && px < p.kw && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                ra[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (ok) ra[i] = *reinterpret_cast<const f32x4_t *>(p.x + aoff[i] + ((long long)khi * p.W + px) * 4);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) rb[i] = *reinterpret_cast<const f32x4_t *>(wrow[i] + kt * 32);
        };
        auto store_lds = [&](int buf) __attribute__((always_inline)) {
            char *sa = smem + buf * A_BYTES;
            char *sb = smem + 2 * A_BYTES + buf * B_BYTES;
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4_t *>(sa + lds_off(lrow + 32 * i, slot)) = ra[i];
#pragma unroll
            for (int i = 0; i < NB; ++i) *reinterpret_cast<f32x4_t *>(sb + lds_off(lrow + 32 * i, slot)) = rb[i];
        };
        auto compute = [&](int buf) __attribute__((always_inline)) {
            const char *sa = smem + buf * A_BYTES;
            const char *sb = smem + 2 * A_BYTES + buf * B_BYTES;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int sl = q * 2 + kgrp;
                f32x4_t fa[MI], fb[NI];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) fa[mi] = *reinterpret_cast<const f32x4_t *>(sa + lds_off(wm * WMT + mi * 32 + l31, sl));
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) fb[ni] = *reinterpret_cast<const f32x4_t *>(sb + lds_off(wn * WN + ni * 32 + l31, sl));
                mfma_group(fa, fb);
            }
        };
        load_tile(0);
        store_lds(0);
        __syncthreads();
        for (int kt = 0; kt < p.nk; ++kt) {
            const int cur = kt & 1;
            const bool more = kt + 1 < p.nk;
            if (more) load_tile(kt + 1);
            compute(cur);
            if (more) store_lds(cur ^ 1);
            __syncthreads();
        }
    }

    // ---- epilogue: the accumulators go through LDS as an fp32 tile; thread (r0, c8) finishes 8 consecutive channels of rows
    // r0 + pass * RPP, in conv_igemm.hip's operation order
    constexpr int TPR = BN / 8;   // threads per row
    constexpr int RPP = NT / TPR; // rows per pass
    constexpr int NPASS = BM / RPP;
    const int c8 = t % TPR;
    const int r0 = t / TPR;
    const int c = n0 + c8 * 8;
    const bool cok = c < p.Cout;
    const bool full = c + 8 <= p.Cout;
    float *ct = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WMT + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kgrp;
                const int col = wn * WN + ni * 32 + l31;
                ct[row * CT_STRIDE + col] = acc[mi][ni][r];
            }
    __syncthreads();
    if (!cok) return;
    const bool post = p.s2 != nullptr;
    float s1[8], b1[8], s2[8], b2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { // (scale / shift are padded to the column tile)
        s1[j] = p.s1[c + j];
        b1[j] = p.b1[c + j];
        s2[j] = post ? p.s2[c + j] : 1.f;
        b2[j] = post ? p.b2[c + j] : 0.f;
    }
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        const int lrow_e = pass * RPP + r0;
        const int m = m0 + lrow_e;
        if (m >= p.M) continue;
        float v[8];
        const f32x4_t q0 = *reinterpret_cast<const f32x4_t *>(ct + lrow_e * CT_STRIDE + c8 * 8);
        const f32x4_t q1 = *reinterpret_cast<const f32x4_t *>(ct + lrow_e * CT_STRIDE + c8 * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = q0[j] * s1[j] + b1[j];
            v[4 + j] = q1[j] * s1[4 + j] + b1[4 + j];
        }
        const long long o = (long long)m * p.Cout + c;
        if (p.res != nullptr && full) {
            const f32x4_t a0 = *reinterpret_cast<const f32x4_t *>(p.res + o), a1 = *reinterpret_cast<const f32x4_t *>(p.res + o + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] += a0[j];
                v[4 + j] += a1[j];
            }
        }
        if (p.relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = relu_keep_nan(v[j]);
        }
        if (post) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * s2[j] + b2[j];
        }
        const f32x4_t o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
        if (p.y_f32 != nullptr) {
            if (full && (p.Cout & 3) == 0) {
                *reinterpret_cast<f32x4_t *>(p.y_f32 + o) = o0;
                *reinterpret_cast<f32x4_t *>(p.y_f32 + o + 4) = o1;
            } else {
                for (int j = 0; j < 8 && c + j < p.Cout; ++j) p.y_f32[o + j] = v[j];
            }
        }
        if (p.y != nullptr && full) {
            const long long oy = (long long)m * p.ldy + c;
            *reinterpret_cast<f32x4_t *>(p.y + oy) = o0;
            *reinterpret_cast<f32x4_t *>(p.y + oy + 4) = o1;
        }
    }
}

template <int BN, int MODE>
constexpr int conv_f32_lds() {
    constexpr int PIPE = 2 * (128 * 128 + BN * 128), EPI = 128 * (BN + 4) * 4;
    return PIPE > EPI ? PIPE : EPI;
}

} // namespace

int conv_f32_launch(wsc_ctx *ctx, const ConvLaunch &p) {
    WSC_CHECK(p.prec == WSC_PREC_F32 && p.operands_match() && !p.x.lo && !p.res.lo && !p.y.lo, WSC_ERR_INVALID,
              "conv (fp32): one plane of fp32 activations");
    WSC_CHECK(p.form != CONV_FORM_STEM_ROWS && !p.x2, WSC_ERR_INVALID,
              "conv (fp32): the padded-stem form and the second input are half-mode paths");
    if (p.form == CONV_FORM_GENERIC) WSC_CHECK(p.Cin % 32 == 0, WSC_ERR_INVALID, "conv (fp32): Cin=%d not a multiple of 32", p.Cin);
    else WSC_CHECK(p.Cin == 4 && p.kw <= (p.form == CONV_FORM_SMALL2 ? 4 : 8), WSC_ERR_INVALID, "conv (fp32): small-Cin mode needs a 4-channel activation");
    WSC_CHECK(p.dil >= 1 && (p.dil == 1 || p.form == CONV_FORM_GENERIC), WSC_ERR_INVALID, "conv (fp32): dilation %d needs a generic layer", p.dil);
    WSC_CHECK(p.CoutPad % 64 == 0 && p.Cout <= p.CoutPad, WSC_ERR_INVALID, "conv (fp32): CoutPad=%d not a multiple of 64", p.CoutPad);
    const int ldy = p.ldy > 0 ? p.ldy : p.Cout;
    WSC_CHECK((!p.y && !p.res) || (p.Cout % 8 == 0 && ldy % 4 == 0), WSC_ERR_INVALID,
              "conv (fp32): an activation output / residual needs Cout=%d in multiples of 8", p.Cout);
    WSC_CHECK(p.y || p.y_f32 != nullptr, WSC_ERR_INVALID, "conv (fp32): no output");
    const ConvKLayout k = conv_k_layout(p.kh, p.kw, p.Cin, p.form, p.prec);
    ConvF32Args a = {};
    a.x = p.x.f32(); a.w = (const float *)p.w;
    a.s1 = p.s1; a.b1 = p.b1; a.s2 = p.s2; a.b2 = p.b2;
    a.res = p.res.f32();
    a.y = p.y.f32(); a.y_f32 = p.y_f32;
    a.H = p.H; a.W = p.W; a.Cin = p.Cin; a.Ho = p.Ho; a.Wo = p.Wo; a.Cout = p.Cout;
    a.ldy = ldy;
    a.kh = p.kh; a.kw = p.kw; a.stride = p.stride; a.pad = p.pad; a.relu = p.relu; a.dil = p.dil;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    WSC_CHECK(M < (1ll << 31) - 256, WSC_ERR_INVALID, "conv (fp32): %lld output pixels", M);
    a.M = (int)M;
    a.HoWo = p.Ho * p.Wo;
    conv_fastdiv((unsigned)(a.HoWo > 0 ? a.HoWo : 1), &a.div_howo_mul, &a.div_howo_s1, &a.div_howo_s2);
    conv_fastdiv((unsigned)(p.Wo > 0 ? p.Wo : 1), &a.div_wo_mul, &a.div_wo_s1, &a.div_wo_s2);
    a.nk = k.nk; a.Kw = k.Kw;
    a.zero = (const float *)ctx->zero_page;
    if (a.M == 0) return WSC_OK;
    const int BN = conv_tile_bn(p.CoutPad);
    a.ntiles_n = p.CoutPad / BN;
    a.nblocks = ((a.M + 127) / 128) * a.ntiles_n;
    void (*kernel)(ConvF32Args);
    int lds, cls;
    auto pick = [&](auto bn) {
        constexpr int B = decltype(bn)::value;
        lds = conv_f32_lds<B, 0>();
        if (p.form == CONV_FORM_GENERIC) { kernel = conv_f32_kernel<B, 0>; cls = B == 128 ? WSC_K_CONV128 : WSC_K_CONV64; }
        else { kernel = p.form == CONV_FORM_SMALL2 ? conv_f32_kernel<B, 1> : conv_f32_kernel<B, 2>; cls = WSC_K_CONV_SMALLCIN; }
    };
    if (BN == 128) pick(std::integral_constant<int, 128>{});
    else pick(std::integral_constant<int, 64>{});
    WSC_TRY(wsc_set_max_dynamic_lds(ctx, reinterpret_cast<const void *>(kernel), lds));
    // algorithmic FLOPs, as conv_igemm_launch counts them
    const double flops = 2.0 * a.M * a.Cout * (p.form == CONV_FORM_GENERIC ? (double)p.kh * p.kw * p.Cin : (double)p.kh * p.kw * 3);
    WscKernelTimer timer(ctx, cls, flops);
    hipLaunchKernelGGL(kernel, dim3(a.nblocks), dim3(256), lds, ctx->stream, a);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}
