// seg_grad.hip -- the kernels of the DeepLab-VGG16 backward pass (wsc_net_backward_seg, net.hip): everything in exact fp32,
// whatever the net's forward precision (gradients of 1e-3 ... 1e-7 per element are below what an IEEE-half plane keeps).
//
//   weight gradient   dW[r][s][ci][co] = sum_{n, ho, wo} x[n][ho - pad + r dil][wo - pad + s dil][ci] dz[n][ho][wo][co]
//                     (stride 1, SAME: pad = dil (k - 1) / 2), one GEMM per tap: Cin x Cout with K = the N H W pixels, fp32
//                     operands on v_mfma_f32_32x32x2_f32 -- bit for bit a pixel-ordered fmaf chain per element and K slice.
//                     Both operands are pixel-major with the channels contiguous, so the LDS image of a K-step (32 pixels) is
//                     [pixel][channel] as it lies in HBM and a lane's fragment element tile[k = l >> 5][i = l & 31] is one
//                     ds_read_b32: the 32 lanes of a half-wave read 32 consecutive floats; the k = 1 half reads one row (a
//                     multiple of 256 bytes = all 64 banks) further on, i.e. the banks of the k = 0 half -- free of conflicts
//                     only if the LDS serves a ds_read_b32 one half-wave at a time, which is ASSUMED, not measured (16 (1 + NI)
//                     such reads per K-step stand against 16 NI MFMAs of 64 cycles).  Staged by global_load_lds_dwordx4 (two buffers, one K-step ahead), taps outside
//                     the image, pixels past the end and columns past Cout from ctx->zero_page.  Parallelism is split-K: slice s
//                     of a tile owns K-steps [s nk / S, (s + 1) nk / S) and writes its own fp32 slab; wgrad_reduce_kernel sums
//                     the slabs IN SLICE ORDER.  No atomic, no arrival counter: two calls give the same bits.  A tap that is
//                     outside the image for every pixel (dil >= the map size: 8 of fc6's 9 taps) gets no block and an exact 0.0.
//       Cin = 3       (conv1_1) the 27 (tap, channel) pairs are ONE 32-row operand gathered on the fly (register staging)
//       Cout <= 32    (fc8) a 32-column tile, zero-filled in LDS past Cout (register staging: its rows are not 16-byte aligned)
//   ReLU mask + bias  dz = dy [y > 0] (fc8: dz = dy), db[c] = sum dz: per block a fixed row range, four row phases summed in
//                     order, then the blocks in order (two launches).
//   data gradient     dX of a stride-1 SAME convolution = the SAME convolution of dz with the 180-degree rotated, channel-
//                     transposed kernel at the same dilation: conv_f32_launch on a kernel packed once (dgrad_pack).
// The pool gradients are in pool.hip.  Per-launch MFMA issue is 16 NI x 64 cycles against BM / 8 + BN / 8 DMA pieces per K-step;
// the kernel is double-buffered and otherwise untuned.
#include "common.h"

#include <algorithm>

namespace {

struct WgradArgs {
    const float *x, *dz;
    float *slab;
    int H, W, Cin, Cout;
    int M, HW;
    unsigned div_hw_mul, div_hw_s1, div_hw_s2, div_w_mul, div_w_s1, div_w_s2; // exact division (conv_fastdiv)
    int k, dil, pad;
    int nk, splits;                // K-steps of 32 pixels; K slices
    int ntaps;                     // taps with a block (all k k of them in the Cin = 3 form, where a block covers every tap)
    unsigned long long taps;       // their r k + s, 4 bits each
    int tiles_ci, tiles_co;
    long long slab_stride;         // k k Cin Cout
    const float *zero;
};

__device__ __forceinline__ void decode_pixel(const WgradArgs &p, int m, int &n, int &ho, int &wo) {
    const unsigned t1 = __umulhi(p.div_hw_mul, (unsigned)m);
    n = (int)((t1 + (((unsigned)m - t1) >> p.div_hw_s1)) >> p.div_hw_s2);
    const int rem = m - n * p.HW;
    const unsigned t2 = __umulhi(p.div_w_mul, (unsigned)rem);
    ho = (int)((t2 + (((unsigned)rem - t2) >> p.div_w_s1)) >> p.div_w_s2);
    wo = rem - ho * p.W;
}

// BM x BN tile of one tap's Cin x Cout product (GATHER_A: of the [27 -> 32] x Cout product of the Cin = 3 form), one K slice.
// Waves WM x WN, 32 x 32 NI per wave.
template <int BM, int BN, bool GATHER_A, bool SCALAR_B>
__global__ __launch_bounds__((BM / 32) * (BN >= 64 ? 2 : 1) * 64) void wgrad_kernel(WgradArgs p) {
    constexpr int WM = BM / 32, WN = BN >= 64 ? 2 : 1, NW = WM * WN, NT = NW * 64, NI = BN / (32 * WN);
    constexpr int A_BYTES = 32 * BM * 4, B_BYTES = 32 * BN * 4;
    constexpr int A_REGS = 32 * BM / NT, B_REGS = 32 * BN / NT; // register-staged elements per thread
    static_assert(!(GATHER_A && BM != 32) && !(SCALAR_B && BN != 32), "register-staged operands are 32 wide");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6); // wave-uniform: LDS DMA destinations stay in SGPRs
    const int wm = wv / WN, wn = wv - wm * WN;
    const int l31 = lane & 31, kgrp = lane >> 5;

    int b = blockIdx.x;
    const int tco = b % p.tiles_co; b /= p.tiles_co;
    const int tci = b % p.tiles_ci; b /= p.tiles_ci;
    const int tl = b % p.ntaps;
    const int slice = b / p.ntaps;
    const int tap = (int)((p.taps >> (4 * tl)) & 15);
    const int tr = tap / p.k, ts = tap - tr * p.k;
    const int dh = tr * p.dil - p.pad, dw = ts * p.dil - p.pad;
    const int ci0 = tci * BM, co0 = tco * BN;
    const int kt0 = (int)((long long)slice * p.nk / p.splits), kt1 = (int)((long long)(slice + 1) * p.nk / p.splits);

    f32x16_t acc[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;

    float ra[GATHER_A ? A_REGS : 1], rb[SCALAR_B ? B_REGS : 1];

    // the LDS-DMA pieces (1 KiB = 64 lanes x 16 bytes) of K-step kt: rows of BM / BN floats, 1024 / (4 BM) pixels per piece
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        if constexpr (!GATHER_A) {
            constexpr int LPP = BM / 4, PIECES = BM / 8;
#pragma unroll
            for (int i = 0; i < PIECES / NW; ++i) {
                const int piece = wv * (PIECES / NW) + i;
                const int m = kt * 32 + piece * (64 / LPP) + lane / LPP;
                const float *g = p.zero;
                if (m < p.M) {
                    int n, ho, wo;
                    decode_pixel(p, m, n, ho, wo);
                    const int hi = ho + dh, wi = wo + dw;
                    if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                        g = p.x + ((((long long)n * p.H + hi) * p.W + wi) * p.Cin + ci0 + (lane % LPP) * 4);
                }
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)(smem + buf * A_BYTES + piece * 1024), 16, 0, 0);
            }
        }
        if constexpr (!SCALAR_B) {
            constexpr int LPP = BN / 4, PIECES = BN / 8;
#pragma unroll
            for (int i = 0; i < PIECES / NW; ++i) {
                const int piece = wv * (PIECES / NW) + i;
                const int m = kt * 32 + piece * (64 / LPP) + lane / LPP;
                const int c = co0 + (lane % LPP) * 4;
                const float *g = (m < p.M && c < p.Cout) ? p.dz + ((long long)m * p.Cout + c) : p.zero; // (Cout % 4 == 0 here)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)(smem + 2 * A_BYTES + buf * B_BYTES + piece * 1024), 16, 0, 0);
            }
        }
    };
    // the register-staged operand(s) of K-step kt: element e = t + NT i of the [32 pixels][32] image
    auto load_regs = [&](int kt) __attribute__((always_inline)) {
        if constexpr (GATHER_A) {
#pragma unroll
            for (int i = 0; i < A_REGS; ++i) {
                const int e = t + NT * i;
                const int m = kt * 32 + (e >> 5), row = e & 31; // row = (tap, channel) pair 3 tap + c
                float v = 0.f;
                if (m < p.M && row < 3 * p.k * p.k) {
                    int n, ho, wo;
                    decode_pixel(p, m, n, ho, wo);
                    const int tp = row / 3, c = row - tp * 3;
                    const int r = tp / p.k, s = tp - r * p.k;
                    const int hi = ho + r * p.dil - p.pad, wi = wo + s * p.dil - p.pad;
                    if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) v = p.x[(((long long)n * p.H + hi) * p.W + wi) * 3 + c];
                }
                ra[i] = v;
            }
        }
        if constexpr (SCALAR_B) {
#pragma unroll
            for (int i = 0; i < B_REGS; ++i) {
                const int e = t + NT * i;
                const int m = kt * 32 + (e >> 5), c = co0 + (e & 31);
                rb[i] = (m < p.M && c < p.Cout) ? p.dz[(long long)m * p.Cout + c] : 0.f;
            }
        }
    };
    auto store_regs = [&](int buf) __attribute__((always_inline)) {
        if constexpr (GATHER_A) {
            float *sa = reinterpret_cast<float *>(smem + buf * A_BYTES);
#pragma unroll
            for (int i = 0; i < A_REGS; ++i) sa[t + NT * i] = ra[i];
        }
        if constexpr (SCALAR_B) {
            float *sb = reinterpret_cast<float *>(smem + 2 * A_BYTES + buf * B_BYTES);
#pragma unroll
            for (int i = 0; i < B_REGS; ++i) sb[t + NT * i] = rb[i];
        }
    };

    if (kt0 < kt1) { // (block-uniform; wgrad_plan gives every slice a K-step, an empty one would write zeros)
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
        const unsigned baseA = lds0 + (unsigned)((kgrp * BM + wm * 32 + l31) * 4);
        const unsigned baseB = lds0 + 2 * A_BYTES + (unsigned)((kgrp * BN + wn * 32 * NI + l31) * 4);
        issue(kt0, 0);
        load_regs(kt0);
        store_regs(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kt = kt0; kt < kt1; ++kt) {
            const int cur = (kt - kt0) & 1;
            const bool more = kt + 1 < kt1;
            if (more) {
                issue(kt + 1, cur ^ 1);
                load_regs(kt + 1);
            }
            // Fragment reads as inline asm with their own wait: compiler-visible ds_reads would get an s_waitcnt vmcnt(0) in
            // front while the DMA of the next K-step is in flight (conv_f32.hip).  MFMA j takes pixels 2 j and 2 j + 1.
            const unsigned aA = baseA + cur * A_BYTES, aB = baseB + cur * B_BYTES;
            float fa[16], fb[NI][16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                asm volatile("ds_read_b32 %0, %1" : "=v"(fa[j]) : "v"(aA + (unsigned)(j * 2 * BM * 4)) : "memory");
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    asm volatile("ds_read_b32 %0, %1" : "=v"(fb[ni][j]) : "v"(aB + (unsigned)(j * 2 * BN * 4 + ni * 128)) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j], fb[ni][j], acc[ni], 0, 0, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the next K-step's pieces have landed ...
            if (more) store_regs(cur ^ 1);
            __syncthreads();                                  // ... for every wave, and every read of this buffer is done
        }
    }

    // C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *out = p.slab + (long long)slice * p.slab_stride;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int co = co0 + wn * 32 * NI + ni * 32 + l31;
        if (co >= p.Cout) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kgrp;
            if constexpr (GATHER_A) {
                if (row < 3 * p.k * p.k) out[(long long)row * p.Cout + co] = acc[ni][r];
            } else {
                out[((long long)tap * p.Cin + ci0 + row) * p.Cout + co] = acc[ni][r];
            }
        }
    }
}

// dw[i] = slab 0 [i] + slab 1 [i] + ... in slice order; a tap of `dead` is +0.0 and its slabs are never read
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ slab, int splits, long long n, long long tap_elems,
                                                           unsigned dead, float *__restrict__ dw) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (!((dead >> (int)(i / tap_elems)) & 1u)) {
            s = slab[i];
            for (int k = 1; k < splits; ++k) s += slab[(long long)k * n + i];
        }
        dw[i] = s;
    }
}

// stage 1 of the mask + bias pass: block g owns rows [g R, (g + 1) R); lane tx a channel of every 64-channel group, the four
// waves the rows r % 4; partial[g][c] = ((wave 0 + wave 1) + wave 2) + wave 3
__global__ __launch_bounds__(256) void relu_bias_grad_kernel(const float *__restrict__ y, const float *__restrict__ dy, long long M, int C,
                                                             long long R, float scale, float *__restrict__ dz, float *__restrict__ partial) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * R;
    const long long r1 = r0 + R < M ? r0 + R : M;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + tx;
        float s = 0.f;
        if (c < C)
            for (long long r = r0 + ty; r < r1; r += 4) {
                const long long o = r * C + c;
                float v = dy[o];
                if (y != nullptr) v = y[o] > 0.f ? __fmul_rn(v, scale) : 0.f; // (one rounding, never fused into the sum; 1.0f: exact)
                if (dz != nullptr) dz[o] = v;
                s += v;
            }
        red[ty][tx] = s;
        __syncthreads();
        if (ty == 0 && c < C) partial[(long long)blockIdx.x * C + c] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void bias_grad_finish_kernel(const float *__restrict__ partial, int G, int C, float *__restrict__ db) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = partial[c];
    for (int g = 1; g < G; ++g) s += partial[(long long)g * C + c];
    db[c] = s;
}

// dst[m][0 .. Cd) = src[m][0 .. min(Cs, Cd)), zeros beyond (fc8's gradient padded to 32 channels; the NHWC4 input without its
// fourth channel)
__global__ __launch_bounds__(256) void copy_channels_kernel(const float *__restrict__ src, long long M, int Cs, int Cd, float *__restrict__ dst) {
    const long long total = M * Cd;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / Cd;
        const int c = (int)(i - m * Cd);
        dst[i] = c < Cs ? src[m * Cs + c] : 0.f;
    }
}

} // namespace

int wgrad_plan(const wsc_ctx *ctx, int N, int H, int W, int Cin, int Cout, int k, int dil, int splits, WgradPlan *pl) {
    WSC_CHECK(N > 0 && H > 0 && W > 0 && (k == 1 || k == 3) && dil >= 1, WSC_ERR_INVALID, "weight gradient: %d x %d x %d, kernel %d, dilation %d", N,
              H, W, k, dil);
    WSC_CHECK(Cin == 3 || (Cin > 0 && Cin % 64 == 0), WSC_ERR_INVALID, "weight gradient: Cin=%d (3 or a multiple of 64)", Cin);
    WSC_CHECK((Cout >= 2 && Cout <= 32 && Cin != 3) || (Cout > 0 && Cout % 64 == 0), WSC_ERR_INVALID,
              "weight gradient: Cout=%d (2 .. 32 behind a wide layer, or a multiple of 64)", Cout);
    WSC_CHECK(splits >= 0, WSC_ERR_INVALID, "weight gradient: %d K slices", splits);
    const long long M = (long long)N * H * W;
    WSC_CHECK(M < (1ll << 31) - 64, WSC_ERR_INVALID, "weight gradient: %lld pixels", M);
    pl->M = (int)M;
    pl->nk = (int)((M + 31) / 32);
    pl->pad = dil * (k - 1) / 2;
    pl->small_cin = Cin == 3;
    pl->bn = (pl->small_cin || Cout <= 64) ? (Cout <= 32 ? 32 : 64) : 128; // (the Cin = 3 form has the 64-column tile only)
    pl->tiles_ci = pl->small_cin ? 1 : Cin / 64;
    pl->tiles_co = (Cout + pl->bn - 1) / pl->bn;
    pl->taps = 0;
    pl->ntaps = 0;
    pl->dead = 0;
    for (int r = 0; r < k; ++r)
        for (int s = 0; s < k; ++s) {
            const int dh = r * dil - pl->pad, dw = s * dil - pl->pad;
            const bool live = dh > -H && dh < H && dw > -W && dw < W; // inside the image for some output pixel
            if (!live) pl->dead |= 1u << (r * k + s);
            else if (!pl->small_cin) pl->taps |= (unsigned long long)(r * k + s) << (4 * pl->ntaps++);
        }
    if (pl->small_cin) pl->ntaps = 1; // one block covers every (tap, channel) row; a dead tap's rows sum zeros
    const long long tiles = (long long)pl->ntaps * pl->tiles_ci * pl->tiles_co;
    if (splits == 0) { // blocks ~ 1 - 2 x the CU count
        const long long want = (2ll * (ctx->num_cus > 0 ? ctx->num_cus : 256) + tiles - 1) / tiles;
        splits = (int)std::min<long long>(std::max<long long>(want, 1), 256);
    }
    splits = std::min(splits, pl->nk); // (a slice beyond the K-steps would only write a slab of zeros)
    pl->splits = splits;
    pl->out_elems = (long long)k * k * Cin * Cout;
    pl->slab_elems = pl->out_elems * splits;
    return WSC_OK;
}

int wgrad_launch(wsc_ctx *ctx, const WgradPlan &pl, const float *x, const float *dz, int H, int W, int Cin, int Cout, int k, int dil,
                 float *slab, float *dw) {
    WgradArgs a = {};
    a.x = x; a.dz = dz; a.slab = slab;
    a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.M = pl.M; a.HW = H * W;
    conv_fastdiv((unsigned)a.HW, &a.div_hw_mul, &a.div_hw_s1, &a.div_hw_s2);
    conv_fastdiv((unsigned)W, &a.div_w_mul, &a.div_w_s1, &a.div_w_s2);
    a.k = k; a.dil = dil; a.pad = pl.pad;
    a.nk = pl.nk; a.splits = pl.splits;
    a.ntaps = pl.ntaps; a.taps = pl.taps;
    a.tiles_ci = pl.tiles_ci; a.tiles_co = pl.tiles_co;
    a.slab_stride = pl.out_elems;
    a.zero = (const float *)ctx->zero_page;
    const long long blocks = (long long)pl.ntaps * pl.tiles_ci * pl.tiles_co * pl.splits;
    WSC_CHECK(blocks < (1ll << 31), WSC_ERR_INVALID, "weight gradient: %lld blocks", blocks);
    WscKernelTimer timer(ctx, WSC_K_WGRAD, 2.0 * pl.M * (double)pl.out_elems);
    if (blocks > 0) {
        // (a slice writes every live element of its slab: the tiles cover Cin x Cout of every live tap)
        if (pl.small_cin)
            hipLaunchKernelGGL((wgrad_kernel<32, 64, true, false>), dim3((unsigned)blocks), dim3(128), 2 * (32 * 32 + 32 * 64) * 4, ctx->stream, a);
        else if (pl.bn == 32)
            hipLaunchKernelGGL((wgrad_kernel<64, 32, false, true>), dim3((unsigned)blocks), dim3(128), 2 * (32 * 64 + 32 * 32) * 4, ctx->stream, a);
        else if (pl.bn == 64)
            hipLaunchKernelGGL((wgrad_kernel<64, 64, false, false>), dim3((unsigned)blocks), dim3(256), 2 * (32 * 64 + 32 * 64) * 4, ctx->stream, a);
        else
            hipLaunchKernelGGL((wgrad_kernel<64, 128, false, false>), dim3((unsigned)blocks), dim3(256), 2 * (32 * 64 + 32 * 128) * 4, ctx->stream, a);
        WSC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(wsc_grid_for(pl.out_elems)), dim3(256), 0, ctx->stream, slab, pl.splits, pl.out_elems,
                       (long long)Cin * Cout, pl.dead, dw);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int relu_bias_grad_blocks(long long M) { return (int)std::min<long long>(std::max<long long>((M + 63) / 64, 1), 1024); }

int launch_relu_bias_grad(wsc_ctx *ctx, const float *y, const float *dy, long long M, int C, float scale, float *dz, float *partial,
                          float *db) {
    WSC_CHECK(M > 0 && C > 0, WSC_ERR_INVALID, "mask + bias gradient: %lld x %d", M, C);
    const int G = relu_bias_grad_blocks(M);
    const long long R = (M + G - 1) / G;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (double)M * C * 4 * (1 + (y != nullptr) + (dz != nullptr)));
    hipLaunchKernelGGL(relu_bias_grad_kernel, dim3(G), dim3(256), 0, ctx->stream, y, dy, M, C, R, scale, dz, partial);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(bias_grad_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, ctx->stream, partial, G, C, db);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_copy_channels(wsc_ctx *ctx, const float *src, long long M, int Cs, int Cd, float *dst) {
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (double)M * (Cs + Cd) * 4);
    hipLaunchKernelGGL(copy_channels_kernel, dim3(wsc_grid_for(M * Cd)), dim3(256), 0, ctx->stream, src, M, Cs, Cd, dst);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

void dgrad_pack(const float *w_hwio, int k, int Cin, int Cout, std::vector<float> *packed) {
    const int Cz = dgrad_cz(Cout), rows = conv_cout_pad(Cin);
    const ConvKLayout lay = conv_k_layout(k, k, Cz, CONV_FORM_GENERIC, WSC_PREC_F32);
    packed->assign((size_t)rows * lay.Kw, 0.f);
    for (int r = 0; r < k; ++r)
        for (int s = 0; s < k; ++s)
            for (int ci = 0; ci < Cin; ++ci)
                for (int co = 0; co < Cout; ++co)
                    (*packed)[(size_t)ci * lay.Kw + lay.index(co, r, s)] = w_hwio[(((size_t)(k - 1 - r) * k + (k - 1 - s)) * Cin + ci) * Cout + co];
}

int dgrad_launch(wsc_ctx *ctx, const float *dz, const float *w_packed, const float *ones, const float *zeros, int N, int H, int W, int Cin,
                 int Cout, int k, int dil, const float *sum_with, float *dx) {
    ConvLaunch L = {};
    L.x.hi = (void *)dz; L.x.prec = WSC_PREC_F32;
    L.w = w_packed; L.s1 = ones; L.b1 = zeros;
    if (sum_with) { L.res.hi = (void *)sum_with; L.res.prec = WSC_PREC_F32; }
    L.y_f32 = dx;
    L.N = N; L.H = H; L.W = W; L.Ho = H; L.Wo = W;
    L.Cin = dgrad_cz(Cout); L.Cout = Cin; L.CoutPad = conv_cout_pad(Cin);
    L.kh = L.kw = k; L.stride = 1; L.pad = dil * (k - 1) / 2; L.dil = dil;
    L.form = CONV_FORM_GENERIC; L.prec = WSC_PREC_F32;
    return conv_f32_launch(ctx, L);
}

// ---- the per-layer entries: float32 NHWC in and out, the launchers of the backward pass unchanged --------------------------------
extern "C" {

int wsc_conv2d_wgrad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int Cin, int Cout, int k, int dil,
                          int splits, float *dw_dev, float *db_dev) {
    WSC_CHECK(ctx && x_dev && dy_dev && dw_dev && db_dev, WSC_ERR_INVALID, "wsc_conv2d_wgrad_nhwc: null argument");
    WgradPlan pl;
    WSC_TRY(wgrad_plan(ctx, N, H, W, Cin, Cout, k, dil, splits, &pl));
    WSC_HIP(hipSetDevice(ctx->device));
    const size_t partial_bytes = (size_t)relu_bias_grad_blocks(pl.M) * Cout * sizeof(float);
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, (size_t)pl.slab_elems * sizeof(float) + partial_bytes, &ws));
    float *slab = (float *)ws, *partial = slab + pl.slab_elems;
    WSC_TRY(wgrad_launch(ctx, pl, x_dev, dy_dev, H, W, Cin, Cout, k, dil, slab, dw_dev));
    return launch_relu_bias_grad(ctx, nullptr, dy_dev, pl.M, Cout, 1.0f, nullptr, partial, db_dev);
}

int wsc_conv2d_dgrad_nhwc(wsc_ctx *ctx, const float *dy_dev, const float *w_host, int N, int H, int W, int Cin, int Cout, int k, int dil,
                          float *dx_dev) {
    WSC_CHECK(ctx && dy_dev && w_host && dx_dev, WSC_ERR_INVALID, "wsc_conv2d_dgrad_nhwc: null argument");
    WSC_CHECK(N > 0 && H > 0 && W > 0 && (k == 1 || k == 3) && dil >= 1 && Cin > 0 && Cin % 64 == 0 && Cout >= 1, WSC_ERR_INVALID,
              "wsc_conv2d_dgrad_nhwc: %d x %d x %d, Cin=%d (a multiple of 64), Cout=%d, kernel %d, dilation %d", N, H, W, Cin, Cout, k, dil);
    WSC_HIP(hipSetDevice(ctx->device));
    std::vector<float> packed;
    dgrad_pack(w_host, k, Cin, Cout, &packed);
    const int Cz = dgrad_cz(Cout), rows = conv_cout_pad(Cin);
    const size_t M = (size_t)N * H * W;
    std::vector<float> vec(2 * (size_t)rows, 0.f);
    for (int i = 0; i < rows; ++i) vec[i] = 1.f;
    const size_t wb = (packed.size() * sizeof(float) + 255) / 256 * 256, vb = (vec.size() * sizeof(float) + 255) / 256 * 256;
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, wb + vb + M * Cz * sizeof(float), &ws));
    char *p = (char *)ws;
    float *w_dev = (float *)p, *vec_dev = (float *)(p + wb), *dz = (float *)(p + wb + vb);
    WSC_HIP(hipStreamSynchronize(ctx->stream)); // (the workspace may still be read by earlier work of the stream)
    WSC_HIP(hipMemcpy(w_dev, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    WSC_HIP(hipMemcpy(vec_dev, vec.data(), vec.size() * sizeof(float), hipMemcpyHostToDevice));
    const float *dz_in = dy_dev;
    if (Cz != Cout) {
        WSC_TRY(launch_copy_channels(ctx, dy_dev, (long long)M, Cout, Cz, dz));
        dz_in = dz;
    }
    return dgrad_launch(ctx, dz_in, w_dev, vec_dev, vec_dev + rows, N, H, W, Cin, Cout, k, dil, nullptr, dx_dev);
}

static int relu_bias_grad_entry(const char *fn, wsc_ctx *ctx, const float *y_dev, const float *dy_dev, long long M, int C, float scale,
                                float *dz_dev, float *db_dev) {
    WSC_CHECK(ctx && dy_dev && dz_dev && db_dev, WSC_ERR_INVALID, "%s: null argument", fn);
    WSC_CHECK(M > 0 && C > 0, WSC_ERR_INVALID, "%s: %lld x %d", fn, M, C);
    WSC_CHECK(scale >= 1.f && scale < INFINITY, WSC_ERR_INVALID, "%s: scale=%g is not 1 / (1 - drop_prob) of a drop_prob in [0, 1)", fn,
              (double)scale);
    WSC_HIP(hipSetDevice(ctx->device));
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, (size_t)relu_bias_grad_blocks(M) * C * sizeof(float), &ws));
    return launch_relu_bias_grad(ctx, y_dev, dy_dev, M, C, scale, dz_dev, (float *)ws, db_dev);
}

int wsc_relu_bias_grad(wsc_ctx *ctx, const float *y_dev, const float *dy_dev, long long M, int C, float *dz_dev, float *db_dev) {
    return relu_bias_grad_entry("wsc_relu_bias_grad", ctx, y_dev, dy_dev, M, C, 1.0f, dz_dev, db_dev);
}

int wsc_relu_bias_grad_scaled(wsc_ctx *ctx, const float *y_dev, const float *dy_dev, long long M, int C, float scale, float *dz_dev,
                              float *db_dev) {
    return relu_bias_grad_entry("wsc_relu_bias_grad_scaled", ctx, y_dev, dy_dev, M, C, scale, dz_dev, db_dev);
}

} // extern "C"
