// irn_grad.hip -- the non-GEMM kernels of the backward pass of the IRNet heads (wsc_net_backward_edge, net.hip).  A head is
//   Conv2d(1x1, bias=False[, stride 2]) -> GroupNorm -> [bilinear upsample] -> ReLU -> crop -> channel slice of a concat buffer
// (irn_kernels.hip has the forward kernels).  Everything here is exact fp32 or double whatever the net's forward precision, for
// the reason at the top of seg_grad.hip; no floating-point atomic, every sum in one fixed order: two calls give the same bits.
//
//   ReLU mask + upsample adjoint   dy[n][y][x][c] = sum over the destination pixels (ho, wo) of the crop whose bilinear stencil
//                     touches source pixel (y, x), in ascending (ho, wo) order, of w(ho, y) w(wo, x) dcat[n][ho][wo][coff + c]
//                     where the TAPED concat value at that position is > 0 (an exact 0 masks, as torch's ReLU does).  Gather
//                     form: a thread owns source elements.  w are the float weights hy, ly, hx, lx gn_apply_kernel forms
//                     (src = (dst + 0.5) / up - 0.5 clamped at 0, y1 = y0 at the last row); at the last row / column both
//                     taps of a destination land on the one source pixel and both count (w = hy + ly).  For up in {1, 2, 4}
//                     every weight is a multiple of 1 / 8, so a product of two is exact and each term costs one rounding (the
//                     fmaf into the running sum).  The forward applies GroupNorm's affine map after the interpolation; both
//                     are linear, so the adjoint is the one of interpolating the GroupNorm output.
//   GroupNorm backward  with xh = (z - mean) rstd from the TAPED float statistics, per (sample, channel) A = sum_p dy and
//                     B = sum_p dy xh in double: pass 1 sums the pixels of a chunk (GNG_CHUNK, four row phases added in order),
//                     a second kernel adds the chunks in order, the finish step forms dbeta[c] = sum_n A, dgamma[c] = sum_n B and per (sample,
//                     group) m1 = sum_c gamma_c A / m, m2 = sum_c gamma_c B / m (m = Cg H W); pass 2 writes
//                     dz = rstd (gamma_c dy - m1 - xh m2), formed in double and rounded once.
//   strided rows      x[:, ::s, ::s, :] as a dense operand of the weight-gradient GEMM (the stride-2 heads of VGG16 and M7)
//   dp_out's gradient [N][2][Hd][Wd] -> [N Hd Wd][Cd] pixel-major, zeros past channel 1
//   channel mean      the closing dp_mean pass (train_irn.py:148-164, wsc_channel_mean_nchw of net.hip): x [N][C][HW] -> mean[c] over
//                     (n, p) in double: block (b, c) sums the items b 256 + t + k B 256 of channel c, each thread in ascending k,
//                     the block in block_sum's order; partial[c][b] to HBM; the block of a channel that arrives last (common.h's
//                     ticket, one per channel) adds the partials in block order, divides by N HW and subtracts sub[c].  An item
//                     is four consecutive floats of one plane (added in order) where HW % 4 == 0 and x is 16-byte aligned, else
//                     one float.
// The element kernels have a 16-byte form (four channels per thread) and a scalar form with the same expressions per element.
#include "common.h"

#include <algorithm>

namespace {

constexpr int GNG_CHUNK = 256; // pixels per block of pass 1
constexpr int CM_BLOCK = 256;  // threads of the channel mean

struct UpGradArgs {
    const float *dcat, *cat; // [N][Hd][Wd][Ctot]
    float *dy;               // [N][H][W][C]
    int N, H, W, C, up, Hd, Wd, Ctot, coff;
};

// the forward's taps of destination index d on an axis of `size` source pixels -> the weight source index s receives
__device__ __forceinline__ float up_weight(int d, int s, int size, float inv) {
    float sf = ((float)d + 0.5f) * inv - 0.5f;
    sf = sf < 0.f ? 0.f : sf;
    const int i0 = (int)sf;
    const int i1 = i0 + (i0 < size - 1 ? 1 : 0);
    const float l = sf - (float)i0, h = 1.f - l;
    return (i0 == s ? h : 0.f) + (i1 == s ? l : 0.f);
}

template <int VEC>
__global__ __launch_bounds__(256) void relu_up_grad_kernel(UpGradArgs a) {
    const int CV = a.C / VEC;
    const long long total = (long long)a.N * a.H * a.W * CV;
    const float inv = 1.0f / (float)a.up;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % CV) * VEC;
        long long t = i / CV;
        const int x = (int)(t % a.W);
        t /= a.W;
        const int y = (int)(t % a.H);
        const int n = (int)(t / a.H);
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
        // destinations whose stencil can touch (y, x): up = 1 the pixel itself, else [up s - up / 2, up s + 3 up / 2)
        const int h0 = a.up == 1 ? y : max(a.up * y - a.up / 2, 0), h1 = a.up == 1 ? y + 1 : a.up * y + 3 * a.up / 2;
        const int w0 = a.up == 1 ? x : max(a.up * x - a.up / 2, 0), w1 = a.up == 1 ? x + 1 : a.up * x + 3 * a.up / 2;
        for (int ho = h0; ho < min(h1, a.Hd); ++ho) {
            const float wy = a.up == 1 ? 1.f : up_weight(ho, y, a.H, inv);
            if (wy == 0.f) continue;
            for (int wo = w0; wo < min(w1, a.Wd); ++wo) {
                const float wx = a.up == 1 ? 1.f : up_weight(wo, x, a.W, inv);
                if (wx == 0.f) continue;
                const float w = wy * wx; // exact: multiples of 1 / 8 in [0, 1]
                const long long o = (((long long)n * a.Hd + ho) * a.Wd + wo) * a.Ctot + a.coff + c0;
                if constexpr (VEC == 4) {
                    const f32x4_t v = *reinterpret_cast<const f32x4_t *>(a.cat + o);
                    const f32x4_t g = *reinterpret_cast<const f32x4_t *>(a.dcat + o);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (v[j] > 0.f) acc[j] = __builtin_fmaf(w, g[j], acc[j]);
                } else {
                    if (a.cat[o] > 0.f) acc[0] = __builtin_fmaf(w, a.dcat[o], acc[0]);
                }
            }
        }
        float *out = a.dy + (((long long)n * a.H + y) * a.W + x) * a.C + c0;
        if constexpr (VEC == 4) {
            f32x4_t r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = acc[j];
            *reinterpret_cast<f32x4_t *>(out) = r;
        } else {
            out[0] = acc[0];
        }
    }
}

// pass 1: block (n, chunk); lane tx a channel of every 64-channel group, the four waves the pixels p % 4 of the chunk;
// partial[(n nchunk + chunk) C + c] = {A, B} = ((wave 0 + wave 1) + wave 2) + wave 3
__global__ __launch_bounds__(256) void gn_grad_partial_kernel(const float *__restrict__ z, const float *__restrict__ dy,
                                                              const float2 *__restrict__ stats, int HW, int C, int G, int nchunk,
                                                              double2 *__restrict__ partial) {
    __shared__ double red[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = blockIdx.x / nchunk, chunk = blockIdx.x - n * nchunk;
    const int Cg = C / G;
    const int p0 = chunk * GNG_CHUNK, p1 = min(p0 + GNG_CHUNK, HW);
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + tx;
        double sa = 0.0, sb = 0.0;
        if (c < C) {
            const float2 st = stats[n * G + c / Cg];
            const double mean = (double)st.x, rstd = (double)st.y;
            for (int p = p0 + ty; p < p1; p += 4) {
                const long long o = ((long long)n * HW + p) * C + c;
                const double g = (double)dy[o];
                sa += g;
                sb += g * (((double)z[o] - mean) * rstd);
            }
        }
        red[0][ty][tx] = sa;
        red[1][ty][tx] = sb;
        __syncthreads();
        if (ty == 0 && c < C)
            partial[((long long)n * nchunk + chunk) * C + c] = make_double2(((red[0][0][tx] + red[0][1][tx]) + red[0][2][tx]) + red[0][3][tx],
                                                                            ((red[1][0][tx] + red[1][1][tx]) + red[1][2][tx]) + red[1][3][tx]);
        __syncthreads();
    }
}

// col[n C + c] = the chunks of (sample n, channel c) added in chunk order
__global__ __launch_bounds__(256) void gn_grad_columns_kernel(const double2 *__restrict__ partial, int N, int C, int nchunk,
                                                              double2 *__restrict__ col) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * C) return;
    const int n = t / C, c = t - n * C;
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        const double2 v = partial[((long long)n * nchunk + k) * C + c];
        sa += v.x;
        sb += v.y;
    }
    col[t] = make_double2(sa, sb);
}

// the finish step: threads [0, C) the channel sums over the samples in sample order, threads [C, C + N G) the group means of
// one sample, its channels in channel order
__global__ __launch_bounds__(256) void gn_grad_finish_kernel(const double2 *__restrict__ col, const float *__restrict__ gamma, int N, int C,
                                                             int G, double m, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                             double2 *__restrict__ ms) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < C) {
        double sa = 0.0, sb = 0.0;
        for (int n = 0; n < N; ++n) {
            const double2 v = col[n * C + t];
            sa += v.x;
            sb += v.y;
        }
        dbeta[t] = (float)sa;
        dgamma[t] = (float)sb;
    } else if (t < C + N * G) {
        const int ng = t - C, n = ng / G, g = ng - n * G, Cg = C / G;
        double s1 = 0.0, s2 = 0.0;
        for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
            const double2 v = col[n * C + c];
            const double ga = (double)gamma[c];
            s1 += ga * v.x;
            s2 += ga * v.y;
        }
        ms[ng] = make_double2(s1 / m, s2 / m);
    }
}

// pass 2
template <int VEC>
__global__ __launch_bounds__(256) void gn_grad_apply_kernel(const float *__restrict__ z, const float *__restrict__ dy,
                                                            const float2 *__restrict__ stats, const float *__restrict__ gamma,
                                                            const double2 *__restrict__ ms, int N, int HW, int C, int G,
                                                            float *__restrict__ dz) {
    const int CV = C / VEC, Cg = C / G;
    const long long total = (long long)N * HW * CV;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % CV) * VEC;
        const long long pix = i / CV;
        const int n = (int)(pix / HW);
        const long long o = pix * C + c0;
        float zv[VEC], gv[VEC], r[VEC];
        if constexpr (VEC == 4) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t *>(z + o), b = *reinterpret_cast<const f32x4_t *>(dy + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) { zv[j] = a[j]; gv[j] = b[j]; }
        } else {
            zv[0] = z[o];
            gv[0] = dy[o];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int c = c0 + j, ng = n * G + c / Cg;
            const float2 st = stats[ng];
            const double2 mm = ms[ng];
            const double rstd = (double)st.y;
            const double xh = ((double)zv[j] - (double)st.x) * rstd;
            r[j] = (float)(rstd * (((double)gamma[c] * (double)gv[j] - mm.x) - xh * mm.y));
        }
        if constexpr (VEC == 4) {
            f32x4_t v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = r[j];
            *reinterpret_cast<f32x4_t *>(dz + o) = v;
        } else {
            dz[o] = r[0];
        }
    }
}

// y[n][ho][wo][0 .. C) = x[n][ho s][wo s][0 .. C), four channels per thread (C a multiple of 4)
__global__ __launch_bounds__(256) void strided_rows_kernel(const float *__restrict__ x, int N, int H, int W, int C4, int s, int Ho, int Wo,
                                                           float *__restrict__ y) {
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long t = i / C4;
        const int wo = (int)(t % Wo);
        t /= Wo;
        const int ho = (int)(t % Ho);
        const int n = (int)(t / Ho);
        reinterpret_cast<f32x4_t *>(y)[i] =
            reinterpret_cast<const f32x4_t *>(x)[(((long long)n * H + (long long)ho * s) * W + (long long)wo * s) * C4 + c];
    }
}

// out[(n, p)][c] = ddp[n][c][p] for c < 2, zeros beyond
__global__ __launch_bounds__(256) void dp_to_nhwc_kernel(const float *__restrict__ ddp, long long M, int HW, int Cd, float *__restrict__ out) {
    const long long total = M * Cd;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / Cd;
        const int c = (int)(i - m * Cd);
        const long long n = m / HW, p = m - n * HW;
        out[i] = c < 2 ? ddp[(n * 2 + c) * HW + p] : 0.f;
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
__global__ __launch_bounds__(CM_BLOCK) void channel_mean_kernel(ChannelMeanArgs a) {
    __shared__ double scratch[CM_BLOCK / 64], fin[CHANNEL_MEAN_MAX_BLOCKS];
    __shared__ int s_last;
    const int tid = threadIdx.x, c = blockIdx.y;
    constexpr int PER = VEC ? 4 : 1;
    const long long items = a.count / PER, per_plane = a.HW / PER; // (VEC: HW % 4 == 0)
    double s[1] = {0.0};
    for (long long i = (long long)blockIdx.x * CM_BLOCK + tid; i < items; i += (long long)gridDim.x * CM_BLOCK) {
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
        ticket_publish();
        s_last = ticket_is_last(a.tickets + c, gridDim.x);
    }
    __syncthreads();
    if (!s_last) return;
    for (unsigned b = tid; b < gridDim.x; b += CM_BLOCK) fin[b] = a.partials[(long long)c * gridDim.x + b];
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) t += fin[b];
        t /= (double)a.count;
        if (a.sub) t -= (double)a.sub[c];
        a.out[c] = t;
    }
}

int check_up_grad(const char *fn, int N, int H, int W, int C, int up, int Hd, int Wd, int Ctot, int coff) {
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0, WSC_ERR_INVALID, "%s: %d x %d x %d x %d", fn, N, H, W, C);
    WSC_CHECK(up == 1 || up == 2 || up == 4, WSC_ERR_INVALID, "%s: upsample factor %d (1, 2 or 4)", fn, up);
    WSC_CHECK(Hd >= 1 && Wd >= 1 && Hd <= H * up && Wd <= W * up, WSC_ERR_INVALID, "%s: crop %d x %d of a %d x %d map", fn, Hd, Wd, H * up,
              W * up);
    WSC_CHECK(coff >= 0 && Ctot >= 1 && coff <= Ctot - C, WSC_ERR_INVALID, "%s: channels [%d, %d + %d) of %d", fn, coff, coff, C, Ctot);
    return WSC_OK;
}

} // namespace

int launch_relu_upsample_grad(wsc_ctx *ctx, const float *dcat, const float *cat, int N, int H, int W, int C, int up, int Hd, int Wd, int Ctot,
                              int coff, float *dy) {
    WSC_TRY(check_up_grad("ReLU + upsample gradient", N, H, W, C, up, Hd, Wd, Ctot, coff));
    UpGradArgs a;
    a.dcat = dcat; a.cat = cat; a.dy = dy;
    a.N = N; a.H = H; a.W = W; a.C = C; a.up = up; a.Hd = Hd; a.Wd = Wd; a.Ctot = Ctot; a.coff = coff;
    const bool vec = C % 4 == 0 && Ctot % 4 == 0 && coff % 4 == 0 && aligned16(dcat) && aligned16(cat) && aligned16(dy);
    const long long items = (long long)N * H * W * (vec ? C / 4 : C);
    const int taps = up == 1 ? 1 : 4 * up * up;
    WscKernelTimer timer(ctx, WSC_K_UPSAMPLE_GRAD, (double)N * H * W * C * 4 * (1 + 2.0 * taps / (up * up)));
    if (vec) hipLaunchKernelGGL(relu_up_grad_kernel<4>, dim3(wsc_grid_for(items)), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(relu_up_grad_kernel<1>, dim3(wsc_grid_for(items)), dim3(256), 0, ctx->stream, a);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

size_t group_norm_grad_partial_bytes(int N, int H, int W, int C) {
    return sizeof(double2) * (size_t)N * ((H * W + GNG_CHUNK - 1) / GNG_CHUNK + 1) * C; // the chunk sums, then the column sums
}

int launch_group_norm_grad(wsc_ctx *ctx, const float *z, const void *stats, const float *gamma, const float *dy, int N, int H, int W, int C,
                           int G, void *partial, void *ms, float *dz, float *dgamma, float *dbeta) {
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && G > 0 && C % G == 0, WSC_ERR_INVALID, "GroupNorm gradient: %d x %d x %d x %d in %d groups", N,
              H, W, C, G);
    const int HW = H * W, nchunk = (HW + GNG_CHUNK - 1) / GNG_CHUNK;
    WscKernelTimer timer(ctx, WSC_K_GN_GRAD, (double)N * HW * C * 4 * 5);
    hipLaunchKernelGGL(gn_grad_partial_kernel, dim3(N * nchunk), dim3(256), 0, ctx->stream, z, dy, (const float2 *)stats, HW, C, G, nchunk,
                       (double2 *)partial);
    WSC_HIP(hipGetLastError());
    double2 *col = (double2 *)partial + (size_t)N * nchunk * C;
    hipLaunchKernelGGL(gn_grad_columns_kernel, dim3((N * C + 255) / 256), dim3(256), 0, ctx->stream, (const double2 *)partial, N, C, nchunk, col);
    WSC_HIP(hipGetLastError());
    hipLaunchKernelGGL(gn_grad_finish_kernel, dim3((C + N * G + 255) / 256), dim3(256), 0, ctx->stream, (const double2 *)col, gamma, N, C, G,
                       (double)HW * (C / G), dgamma, dbeta, (double2 *)ms);
    WSC_HIP(hipGetLastError());
    const bool vec = C % 4 == 0 && aligned16(z) && aligned16(dy) && aligned16(dz);
    const long long items = (long long)N * HW * (vec ? C / 4 : C);
    if (vec)
        hipLaunchKernelGGL(gn_grad_apply_kernel<4>, dim3(wsc_grid_for(items)), dim3(256), 0, ctx->stream, z, dy, (const float2 *)stats, gamma,
                           (const double2 *)ms, N, HW, C, G, dz);
    else
        hipLaunchKernelGGL(gn_grad_apply_kernel<1>, dim3(wsc_grid_for(items)), dim3(256), 0, ctx->stream, z, dy, (const float2 *)stats, gamma,
                           (const double2 *)ms, N, HW, C, G, dz);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_strided_rows_f32(wsc_ctx *ctx, const float *x, int N, int H, int W, int C, int stride, int Ho, int Wo, float *y) {
    WSC_CHECK(C % 4 == 0 && stride >= 1 && (Ho - 1) * stride < H && (Wo - 1) * stride < W && aligned16(x) && aligned16(y), WSC_ERR_INVALID,
              "strided rows: %d x %d x %d at stride %d into %d x %d", H, W, C, stride, Ho, Wo);
    const long long items = (long long)N * Ho * Wo * (C / 4);
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (double)items * 32);
    hipLaunchKernelGGL(strided_rows_kernel, dim3(wsc_grid_for(items)), dim3(256), 0, ctx->stream, x, N, H, W, C / 4, stride, Ho, Wo, y);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int launch_dp_to_nhwc(wsc_ctx *ctx, const float *ddp, int N, int HW, int Cd, float *out) {
    WSC_CHECK(N > 0 && HW > 0 && Cd >= 2, WSC_ERR_INVALID, "displacement gradient: %d x %d into %d channels", N, HW, Cd);
    const long long M = (long long)N * HW;
    WscKernelTimer timer(ctx, WSC_K_GRAD_MISC, (double)M * (2 + Cd) * 4);
    hipLaunchKernelGGL(dp_to_nhwc_kernel, dim3(wsc_grid_for(M * Cd)), dim3(256), 0, ctx->stream, ddp, M, HW, Cd, out);
    WSC_HIP(hipGetLastError());
    return WSC_OK;
}

int channel_mean_launch(wsc_ctx *ctx, const float *x, int N, int C, long long HW, const float *sub_host, double *out) {
    WSC_CHECK(N > 0 && C > 0 && C <= CHANNEL_MEAN_MAX_C && HW > 0, WSC_ERR_INVALID, "channel mean: %d x %d x %lld", N, C, HW);
    const bool vec = HW % 4 == 0 && aligned16(x);
    const long long count = (long long)N * HW, items = vec ? count / 4 : count;
    const int blocks = (int)std::min<long long>(std::max<long long>((items + 4 * CM_BLOCK - 1) / (4 * CM_BLOCK), 1), CHANNEL_MEAN_MAX_BLOCKS);
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
    if (vec) hipLaunchKernelGGL(channel_mean_kernel<true>, dim3(blocks, C), dim3(CM_BLOCK), 0, ctx->stream, a);
    else hipLaunchKernelGGL(channel_mean_kernel<false>, dim3(blocks, C), dim3(CM_BLOCK), 0, ctx->stream, a);
    WSC_HIP(hipGetLastError());
    guard.free_now();
    return WSC_OK;
}

// ---- the per-op entries: float32 NHWC in and out, the launchers of the backward pass unchanged ----------------------------------
extern "C" {

int wsc_relu_upsample_grad_nhwc(wsc_ctx *ctx, const float *dcat_dev, const float *cat_dev, int N, int H, int W, int C, int up, int Hd, int Wd,
                                int Ctot, int coff, float *dy_dev) {
    WSC_CHECK(ctx && dcat_dev && cat_dev && dy_dev, WSC_ERR_INVALID, "wsc_relu_upsample_grad_nhwc: null argument");
    WSC_TRY(check_up_grad("wsc_relu_upsample_grad_nhwc", N, H, W, C, up, Hd, Wd, Ctot, coff));
    WSC_HIP(hipSetDevice(ctx->device));
    return launch_relu_upsample_grad(ctx, dcat_dev, cat_dev, N, H, W, C, up, Hd, Wd, Ctot, coff, dy_dev);
}

int wsc_group_norm_grad_nhwc(wsc_ctx *ctx, const float *z_dev, const float *dy_dev, int N, int H, int W, int C, const float *gamma_host, int G,
                             float eps, float *dz_dev, float *dgamma_dev, float *dbeta_dev) {
    WSC_CHECK(ctx && z_dev && dy_dev && gamma_host && dz_dev && dgamma_dev && dbeta_dev, WSC_ERR_INVALID,
              "wsc_group_norm_grad_nhwc: null argument");
    WSC_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && G > 0 && C % G == 0 && eps > 0.f, WSC_ERR_INVALID,
              "wsc_group_norm_grad_nhwc: %d x %d x %d x %d in %d groups, eps %g", N, H, W, C, G, (double)eps);
    WSC_HIP(hipSetDevice(ctx->device));
    auto lines = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t part_f = lines(group_norm_partial_bytes(N, H, W, G)), stats_b = lines(sizeof(float) * 2 * N * G), vec_b = lines(sizeof(float) * C),
                 part_b = lines(group_norm_grad_partial_bytes(N, H, W, C)), ms_b = lines(sizeof(double2) * N * G);
    void *ws;
    WSC_TRY(wsc_ctx_workspace(ctx, part_f + stats_b + vec_b + part_b + ms_b, &ws));
    char *p = (char *)ws;
    void *part_fwd = p, *stats = p + part_f;
    float *gamma = (float *)(p + part_f + stats_b);
    void *partial = p + part_f + stats_b + vec_b, *ms = p + part_f + stats_b + vec_b + part_b;
    WSC_TRY(wsc_ctx_upload_small(ctx, gamma, gamma_host, sizeof(float) * C));
    WSC_TRY(launch_group_norm_stats(ctx, z_dev, N, H, W, C, G, eps, part_fwd, stats));
    return launch_group_norm_grad(ctx, z_dev, stats, gamma, dy_dev, N, H, W, C, G, partial, ms, dz_dev, dgamma_dev, dbeta_dev);
}

} // extern "C"
