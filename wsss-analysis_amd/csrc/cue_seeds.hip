// cue_seeds.hip -- the 02_cues localization seeds on the device (02_cues/utilities.py:183-278 get_localization_cues /
// get_localization_cues_sec, 02_cues/adp_cues.py:304-339 update_cues; consumer 03a_sec-dsrg/model.py:238-246).
//
//   cue_maps_kernel   one thread per output sample: the gated, channel-selected Grad-CAM map of the NHWC stack that
//                     wsc_net_forward_gradcam leaves, resized to S x S with the sampler of bilinear_kernel (bilerp.h) -- the
//                     bits of "gate on the host, transpose to NCHW, wsc_bilinear_resize"
//   cue_max_kernel    grid (C, B): the maximum of one foreground map into a scratch array [B][C]
//   cue_seed_kernel   one workgroup per image: a mask word per pixel in registers (bit k = localization channel k covers the
//                     pixel), the channel areas in LDS counters, the summed background plane in double in LDS, its 3 x 3
//                     median, the median of rank k by bisection on order-preserving 64-bit keys (one workgroup-wide count per
//                     bit), and the paint pass over the set bits of a word
// Every quantity is an integer, a comparison of exactly formed doubles, or a min / max: nothing depends on the order in which
// threads run or atomics land, and the label map is held to np.array_equal with the oracle of tests/cue_seeds_ref.py.
#include "common.h"
#include "bilerp.h"

namespace {

constexpr int CUE_MAX_L = 32;         // localization channels: one bit each of a pixel's mask word
constexpr int CUE_MAX_PIXELS = 4096;  // H * W: an 8-byte plane per pixel = 32 KiB of the 64 KiB a launch gets without raising the
                                      // dynamic-LDS attribute, and four pixels in the registers of each thread
constexpr int CUE_SEED_THREADS = 1024;
constexpr int CUE_PIX_PER_THREAD = CUE_MAX_PIXELS / CUE_SEED_THREADS; // pixel slot j of thread t is j * CUE_SEED_THREADS + t

__global__ void cue_maps_kernel(const float *__restrict__ cams, int h, int w, int C_all, const int *__restrict__ chan, int C,
                                const float *__restrict__ gate, int S, long long total, float *__restrict__ out) {
    const float sh = (float)h / (float)S, sw = (float)w / (float)S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % S);
        long long r = i / S;
        const int yy = (int)(r % S);
        r /= S; // b * C + c
        const int c = (int)(r % C);
        const long long b = r / C;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(yy, sh, h, y0, y1, ly0, ly1);
        src_index(xx, sw, w, x0, x1, lx0, lx1);
        const float *src = cams + b * h * w * C_all + chan[c];
        // the host gates by multiplying (0 * a negative value is -0), so the same product here
        const float g = gate ? gate[r] : 1.f;
        const float v00 = src[((long long)y0 * w + x0) * C_all], v01 = src[((long long)y0 * w + x1) * C_all];
        const float v10 = src[((long long)y1 * w + x0) * C_all], v11 = src[((long long)y1 * w + x1) * C_all];
        out[i] = gate ? bilerp4(v00 * g, v01 * g, v10 * g, v11 * g, ly0, ly1, lx0, lx1)
                      : bilerp4(v00, v01, v10, v11, ly0, ly1, lx0, lx1);
    }
}

// grid (C, B), 256 threads: mx[b][c] = max over the map (a maximum is exact in any order; NaN is out of contract)
__global__ __launch_bounds__(256) void cue_max_kernel(const float *__restrict__ fg, int HW, float *__restrict__ mx) {
    __shared__ float part[4];
    const size_t map = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const float *src = fg + map * HW;
    float m = src[0];
    for (int p = threadIdx.x; p < HW; p += blockDim.x) m = fmaxf(m, src[p]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) mx[map] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

__device__ __forceinline__ void sort2(double &a, double &b) {
    const double lo = fmin(a, b);
    b = fmax(a, b);
    a = lo;
}
__device__ __forceinline__ double med3(double a, double b, double c) { return fmax(fmin(a, b), fmin(fmax(a, b), c)); }

// Median of nine: sort the three columns, then the median of (largest minimum, median of the medians, smallest maximum).
__device__ __forceinline__ double med9(double v[9]) {
    for (int k = 0; k < 9; k += 3) {
        sort2(v[k], v[k + 1]);
        sort2(v[k + 1], v[k + 2]);
        sort2(v[k], v[k + 1]);
    }
    return med3(fmax(fmax(v[0], v[3]), v[6]), med3(v[1], v[4], v[7]), fmin(fmin(v[2], v[5]), v[8]));
}

// Order-preserving double -> uint64 key (-0 and +0 compare equal as doubles, so both become +0 first).
__device__ __forceinline__ unsigned long long ord_key(double m) {
    if (m == 0.0) m = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(m);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// One workgroup of CUE_SEED_THREADS per image; thread t owns the pixels j * CUE_SEED_THREADS + t and keeps their mask words and
// median keys in registers.  LDS: double plane[HW], double thr[CUE_MAX_L], int area[CUE_MAX_L], int below[64].
__global__ __launch_bounds__(CUE_SEED_THREADS) void cue_seed_kernel(const float *__restrict__ fg, const float *__restrict__ bg,
                                                                    const float *__restrict__ mx, int B, int C, int Cb, int H,
                                                                    int W, double thresh, int per_image_max, int rank,
                                                                    uint8_t *__restrict__ label, int *__restrict__ area_out) {
    extern __shared__ __attribute__((aligned(16))) char cue_lds[];
    const int b = blockIdx.x, HW = H * W, t = threadIdx.x;
    const int has_bg = bg != nullptr, L = C + has_bg;
    const bool lane0 = (t & 63) == 0;
    double *plane = (double *)cue_lds;
    double *thr = plane + HW;
    int *area = (int *)(thr + CUE_MAX_L);
    int *below = area + CUE_MAX_L;

    if (t < CUE_MAX_L) area[t] = 0;
    if (t < 64) below[t] = 0;
    if (t < C) {
        // thresh * max in double, as numpy forms it from a Python float and the float64 maps (utilities.py:218,262 over the
        // batch -- SURVEY Q7; adp_cues.py:322-323 over the image)
        float m = mx[(size_t)b * C + t];
        if (!per_image_max)
            for (int i = 0; i < B; ++i) m = fmaxf(m, mx[(size_t)i * C + t]);
        thr[t] = thresh * (double)m;
    }
    __syncthreads();

    // foreground bits and their areas: one ballot per wave, class and pixel slot, one integer add per wave and class (any order)
    const float *f = fg + (size_t)b * C * HW;
    unsigned wd[CUE_PIX_PER_THREAD] = {};
    for (int c = 0; c < C; ++c) {
        const double th = thr[c];
        float v[CUE_PIX_PER_THREAD];
#pragma unroll
        for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) { // the slots' loads are independent: issued together
            const int p = j * CUE_SEED_THREADS + t;
            v[j] = p < HW ? f[(size_t)c * HW + p] : 0.f;
        }
        int n = 0;
#pragma unroll
        for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) {
            const bool on = j * CUE_SEED_THREADS + t < HW && (double)v[j] > th;
            wd[j] |= (unsigned)on << (c + has_bg);
            n += __popcll(__ballot(on));
        }
        if (lane0 && n) atomicAdd(&area[c + has_bg], n);
    }
    if (has_bg) { // uniform over the workgroup
#pragma unroll
        for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) {
            const int p = j * CUE_SEED_THREADS + t;
            if (p >= HW) continue;
            const float *g = bg + (size_t)b * Cb * HW + p;
            double s = (double)g[0]; // np.sum(axis=0) of the float64 stack: sequential in channel order
#pragma unroll 4
            for (int k = 1; k < Cb; ++k) s += (double)g[(size_t)k * HW];
            plane[p] = s;
        }
        __syncthreads();
        // scipy.ndimage.median_filter(s, 3), mode='reflect': the edge sample is repeated (index -1 -> 0, n -> n - 1)
        unsigned long long key[CUE_PIX_PER_THREAD];
#pragma unroll
        for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) {
            const int p = j * CUE_SEED_THREADS + t;
            key[j] = 0;
            if (p < HW) {
                const int y = p / W, x = p - y * W;
                double v[9];
                for (int dy = -1; dy <= 1; ++dy) {
                    const int yy = min(max(y + dy, 0), H - 1);
                    for (int dx = -1; dx <= 1; ++dx) v[(dy + 1) * 3 + dx + 1] = plane[yy * W + min(max(x + dx, 0), W - 1)];
                }
                key[j] = ord_key(med9(v));
            }
        }
        // The value of rank `rank` among the sorted medians is the largest key v with "fewer than rank + 1 keys are below v":
        // built from its top bit down, one workgroup-wide count per bit (a counter of its own each: one barrier per bit).
        unsigned long long kth = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const unsigned long long cand = kth | (1ull << bit);
            int n = 0;
#pragma unroll
            for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) n += __popcll(__ballot(j * CUE_SEED_THREADS + t < HW && key[j] < cand));
            if (lane0 && n) atomicAdd(&below[bit], n);
            __syncthreads();
            if (below[bit] <= rank) kth = cand;
        }
        int n = 0;
#pragma unroll
        for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) {
            const bool on = j * CUE_SEED_THREADS + t < HW && key[j] < kth; // strict: a constant plane has no background seed
            wd[j] |= (unsigned)on;
            n += __popcll(__ballot(on));
        }
        if (lane0 && n) atomicAdd(&area[0], n);
    }
    __syncthreads();

    // "largest mask first, each paints over what is there" under a stable sort by -area: the covering channel of the smallest
    // area, the higher index among equal areas
    if (area_out && t < L) area_out[(size_t)b * L + t] = area[t];
#pragma unroll
    for (int j = 0; j < CUE_PIX_PER_THREAD; ++j) {
        const int p = j * CUE_SEED_THREADS + t;
        if (p >= HW) continue;
        unsigned w = wd[j];
        int best = 0, best_area = 0x7fffffff;
        while (w) {
            const int k = __ffs(w) - 1;
            w &= w - 1;
            const int a = area[k];
            if (a <= best_area) {
                best_area = a;
                best = k + 1;
            }
        }
        label[(size_t)b * HW + p] = (uint8_t)best;
    }
}

} // namespace

extern "C" {

int wsc_cue_maps(wsc_ctx *ctx, const float *cams_nhwc_dev, int B, int h, int w, int C_all, const int32_t *chan_host, int C,
                 const float *gate_dev, int S, float *out_dev) {
    WSC_CHECK(ctx && cams_nhwc_dev && chan_host && out_dev, WSC_ERR_INVALID, "wsc_cue_maps: null argument");
    WSC_CHECK(B > 0 && h > 0 && w > 0 && C_all > 0 && C > 0 && S > 0, WSC_ERR_INVALID,
              "wsc_cue_maps: B=%d h=%d w=%d C_all=%d C=%d S=%d (sizes must be positive)", B, h, w, C_all, C, S);
    for (int c = 0; c < C; ++c)
        WSC_CHECK(chan_host[c] >= 0 && chan_host[c] < C_all, WSC_ERR_INVALID, "wsc_cue_maps: chan[%d]=%d is no channel of C_all=%d", c,
                  (int)chan_host[c], C_all);
    WSC_HIP(hipSetDevice(ctx->device));
    WscStagedTable tab(ctx);
    const size_t co = tab.add(chan_host, sizeof(int) * (size_t)C);
    WSC_TRY(tab.upload());
    const long long total = (long long)B * C * S * S;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)total * 4 + (double)B * C * h * w * 4);
    hipLaunchKernelGGL(cue_maps_kernel, dim3((unsigned)g), dim3(256), 0, ctx->stream, cams_nhwc_dev, h, w, C_all, tab.at<const int>(co), C,
                       gate_dev, S, total, out_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

int wsc_cue_seeds(wsc_ctx *ctx, const float *fg_dev, const float *bg_dev, int B, int C, int Cb, int H, int W, double thresh,
                  int per_image_max, double bg_fraction, uint8_t *label_dev, int32_t *area_dev) {
    WSC_CHECK(ctx && fg_dev && label_dev, WSC_ERR_INVALID, "wsc_cue_seeds: null argument");
    const int has_bg = bg_dev != nullptr, L = C + has_bg;
    WSC_CHECK(B > 0 && B <= 65535 && C >= 1 && H > 0 && W > 0 && (!has_bg || Cb >= 1), WSC_ERR_INVALID,
              "wsc_cue_seeds: B=%d C=%d Cb=%d H=%d W=%d (sizes must be positive, B <= 65535)", B, C, Cb, H, W);
    WSC_CHECK(L <= CUE_MAX_L, WSC_ERR_INVALID, "wsc_cue_seeds: L=%d localization channels (C=%d%s): at most %d, one bit each", L, C,
              has_bg ? " + background" : "", CUE_MAX_L);
    WSC_CHECK((long long)H * W <= CUE_MAX_PIXELS, WSC_ERR_INVALID,
              "wsc_cue_seeds: H=%d x W=%d = %lld pixels (an image's planes live in LDS: at most %d pixels)", H, W, (long long)H * W,
              CUE_MAX_PIXELS);
    const int HW = H * W;
    // int(bg_fraction * H * W) as Python evaluates it: (bg_fraction * H) * W in double
    const double kd = bg_fraction * (double)H * (double)W;
    WSC_CHECK(bg_fraction >= 0.0 && bg_fraction < 1.0 && (int)kd < HW, WSC_ERR_INVALID,
              "wsc_cue_seeds: bg_fraction=%g (must be in [0, 1): the rank int(bg_fraction * H * W) must index a pixel)", bg_fraction);
    WSC_HIP(hipSetDevice(ctx->device));
    float *mx = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, sizeof(float) * (size_t)B * C, (void **)&mx));
    WscCachedGuard mx_guard(ctx, mx);
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * HW * (4.0 * (2 * C + (has_bg ? Cb : 0)) + 1));
    hipLaunchKernelGGL(cue_max_kernel, dim3(C, B), dim3(256), 0, ctx->stream, fg_dev, HW, mx);
    WSC_HIP(hipGetLastError());
    const size_t lds = (size_t)HW * 8 + CUE_MAX_L * (8 + 4) + 64 * 4;
    hipLaunchKernelGGL(cue_seed_kernel, dim3(B), dim3(CUE_SEED_THREADS), lds, ctx->stream, fg_dev, bg_dev, (const float *)mx, B, C, Cb,
                       H, W, thresh, per_image_max ? 1 : 0, (int)kd, label_dev, area_dev);
    WSC_HIP(hipGetLastError());
    mx_guard.free_now(); // stream-ordered reuse
    return WSC_OK;
}

} // extern "C"
