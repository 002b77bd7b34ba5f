// cls_batch.hip -- the 01_train sample transform on the device: decoded uint8 RGB images in, one batch of network inputs out.
//
// Reference (host, PIL / scipy / numpy, per sample): Keras' ImageDataGenerator behind flow_from_dataframe(target_size=(H, W)),
// configured by 02_cues/dataset.py:28-96 (03c_hsn/dataset.py; 01_train/data_loader.py itself is missing) --
//   load_img(target_size)          PIL Image.resize((W, H), NEAREST), skipped when the image has that size
//   apply_affine_transform         scipy.ndimage.affine_transform(plane, M, off, order=1, mode=fill_mode, cval) on every float32
//                                  H x W plane
//   flip_axis                      columns and / or rows, after the warp
//   standardize                    preprocessing_function, then rescale: ((v - sub[c]) / div) * mul
//   batch_x[i] = x                 float32 [H][W][3] in Keras; [3][H][W] here, the channels R, G, B as cues.utilities._to_nchw
// One launch.  The resized uint8 image never exists: a tap of the warp reads the source through PIL's two nearest-index tables
// (pil_nearest.h, built on the host as for wsc_pil_resize_u8's order 0).
//
// scipy's order-1 warp (ni_interpolation.c, NI_GeometricTransform), restated in double, in its order of operations:
//   c_k = 0; c_k += row * M[k][0]; c_k += col * M[k][1]; c_k += off[k]        (k = 0: the row axis; the offset LAST)
//   c_k = map_coordinate(c_k, n_k, mode)   nearest: a clamp to [0, n - 1]; constant: -1 outside [0, n - 1]; reflect: the period
//                                  2n folded back with a truncated division, then -c - 1 (the grid reflection d c b a | a b c d)
//   c_k <= -1 in either axis: the pixel is cval;  else start = floor(c_k), f = c_k - start, weights w0 = 1 - f, w1 = 1 - w0 (the
//   last weight is one minus the others), the tap indices start and start + 1 mapped by the mode AGAIN (integer reflection; a
//   clamp for nearest and for constant);  t = 0; t += (v[i][j] * wy[i]) * wx[j] in (i, j) order;  one rounding to float32.
// Double because scipy computes in double and the result is held to its bits (tests/cls_batch_ref.py is pinned against scipy,
// the kernel against it); -ffp-contract=off because a fused multiply-add would round once where scipy rounds twice, and because
// the standardisation is three single fp32 roundings (as sgd.hip's steps).
//
// Work: one thread per 16 output bytes.  x_dev is taken as ONE flat array of B * 3 * H * W floats: a thread owns four consecutive
// floats -- they may straddle a row, a plane or a sample (W = 321 is no multiple of 4, nor is 321 * 321), so every element is
// decoded on its own -- and stores them as one 16-byte word; a wave writes 1 KiB of contiguous memory.  The at most three floats
// behind the last whole word, and everything when x_dev is not 16-byte aligned, take the scalar path.  The reads are a gather
// of single bytes (a 500 x 375 source is 0.56 MB).  The coordinate arithmetic is repeated per channel; the alternative -- one
// coordinate computation per pixel and three plane stores, whose 16-byte alignment differs per plane when H * W is odd -- was
// NOT built or measured against this one: the flat form was chosen for its one store path, not on a number.  What this form
// reaches has not been timed yet (profiles/cls_batch.py is the script for it).
#include "common.h"
#include "pil_nearest.h"

#include <math.h>

#include <vector>

namespace {

constexpr int MODE_NEAREST = 0, MODE_REFLECT = 1, MODE_CONSTANT = 2; // WSC_CLS_FILL_*
constexpr int FLAG_WARP = 1, FLAG_FLIP_COLS = 2, FLAG_FLIP_ROWS = 4;
constexpr double MAX_REACH = 1048576.0;                              // 2^20 pixels
constexpr size_t TAB_MAX_INTS = (size_t)1 << 28;                     // int32 indices into the table

struct ClsJob {
    long long src_off;  // bytes of the sample's image in images_dev
    int H0, W0;         // the source
    int ny_off, nx_off; // nearest tables [H] / [W]: resized row / column -> source; < 0: the size is kept
    int flags, pad;
    double a[6];        // M00 M01 M10 M11 off0 off1
};

// map_coordinate of ni_interpolation.c
__device__ __forceinline__ double map_coordinate(double in, int len, int mode) {
    if (in < 0) {
        if (mode == MODE_NEAREST) return 0.0;
        if (mode == MODE_CONSTANT) return -1.0;
        if (len <= 1) return 0.0;
        const long long sz2 = 2LL * len;
        if (in < -(double)sz2) in = (double)(sz2 * (long long)(-in / (double)sz2)) + in;
        return in < -(double)len ? in + (double)sz2 : (in > -1e-15 ? 1e-15 : -in) - 1;
    }
    if (in > len - 1) {
        if (mode == MODE_NEAREST) return (double)(len - 1);
        if (mode == MODE_CONSTANT) return -1.0;
        if (len <= 1) return 0.0;
        const long long sz2 = 2LL * len;
        in -= (double)(sz2 * (long long)(in / (double)sz2));
        if (in >= len) in = (double)sz2 - in - 1;
    }
    return in;
}

// the border mapping of a tap index; the result is inside [0, len) whatever came in
__device__ __forceinline__ int map_tap(int idx, int len, int mode) {
    if (len <= 1) return 0;
    if (mode == MODE_REFLECT) {
        const int s2 = 2 * len;
        if (idx < 0) {
            if (idx < -s2) idx = s2 * (-idx / s2) + idx;
            idx = idx < -len ? idx + s2 : -idx - 1;
        } else if (idx >= len) {
            idx -= s2 * (idx / s2);
            if (idx >= len) idx = s2 - idx - 1;
        }
    }
    return idx < 0 ? 0 : (idx >= len ? len - 1 : idx);
}

// channel c of pixel (r, q) of the RESIZED image, read from the source
__device__ __forceinline__ float source_tap(const ClsJob &job, const uint8_t *__restrict__ im, const int *__restrict__ tab, int r, int q, int c) {
    const int sy = job.ny_off < 0 ? r : tab[job.ny_off + r], sx = job.nx_off < 0 ? q : tab[job.nx_off + q];
    return (float)im[((long long)sy * job.W0 + sx) * 3 + c];
}

// the transformed, not yet standardised value of channel c at (y, x) of the H x W output
__device__ __forceinline__ float cls_value(const ClsJob &job, const uint8_t *__restrict__ im, const int *__restrict__ tab, int H, int W, int mode,
                                           float cval, int c, int y, int x) {
    const int yy = (job.flags & FLAG_FLIP_ROWS) ? H - 1 - y : y, xx = (job.flags & FLAG_FLIP_COLS) ? W - 1 - x : x;
    if (!(job.flags & FLAG_WARP)) return source_tap(job, im, tab, yy, xx, c);
    double c0 = 0.0, c1 = 0.0;
    c0 += (double)yy * job.a[0];
    c0 += (double)xx * job.a[1];
    c0 += job.a[4];
    c1 += (double)yy * job.a[2];
    c1 += (double)xx * job.a[3];
    c1 += job.a[5];
    c0 = map_coordinate(c0, H, mode);
    c1 = map_coordinate(c1, W, mode);
    if (!(c0 > -1.0) || !(c1 > -1.0)) return cval;
    const double f0 = floor(c0), f1 = floor(c1);
    const double y0 = c0 - f0, x0 = c1 - f1;
    const double wy[2] = {1.0 - y0, 1.0 - (1.0 - y0)}, wx[2] = {1.0 - x0, 1.0 - (1.0 - x0)};
    const int r[2] = {map_tap((int)f0, H, mode), map_tap((int)f0 + 1, H, mode)};
    const int q[2] = {map_tap((int)f1, W, mode), map_tap((int)f1 + 1, W, mode)};
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) t += ((double)source_tap(job, im, tab, r[i], q[j], c) * wy[i]) * wx[j];
    return (float)t;
}

struct ClsStd {
    float sub[3], div, mul;
};

// element g of the flat output
struct ClsPos {
    int b, c, y, x;
};

__device__ __forceinline__ ClsPos cls_decode(long long g, int H, int W) {
    const long long hw = (long long)H * W;
    ClsPos p;
    p.b = (int)(g / (3 * hw));
    long long rem = g - (long long)p.b * 3 * hw;
    p.c = (int)(rem / hw);
    rem -= (long long)p.c * hw;
    p.y = (int)(rem / W);
    p.x = (int)(rem - (long long)p.y * W);
    return p;
}

__device__ __forceinline__ float cls_element(const uint8_t *__restrict__ src, const ClsJob *__restrict__ jobs, const int *__restrict__ tab, int H,
                                             int W, int mode, float cval, const ClsStd &st, const ClsPos &p) {
    const ClsJob &job = jobs[p.b];
    const float v = cls_value(job, src + job.src_off, tab, H, W, mode, cval, p.c, p.y, p.x);
    const float sub = p.c == 0 ? st.sub[0] : (p.c == 1 ? st.sub[1] : st.sub[2]);
    return ((v - sub) / st.div) * st.mul;
}

// n_words: the 16-byte words of the flat output the vector path writes (0: x_dev is not 16-byte aligned); the elements from
// 4 * n_words to total are the scalar tail
__global__ __launch_bounds__(256) void cls_batch_kernel(const uint8_t *__restrict__ src, const ClsJob *__restrict__ jobs,
                                                        const int *__restrict__ tab, int H, int W, int mode, float cval, ClsStd st,
                                                        long long n_words, long long total, float *__restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long w = first; w < n_words; w += stride) {
        ClsPos p = cls_decode(4 * w, H, W);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = cls_element(src, jobs, tab, H, W, mode, cval, st, p);
            if (++p.x == W) { // (behind the last element of the batch b == B: not used, 4 * w + 3 < total)
                p.x = 0;
                if (++p.y == H) {
                    p.y = 0;
                    if (++p.c == 3) {
                        p.c = 0;
                        ++p.b;
                    }
                }
            }
        }
        *reinterpret_cast<float4 *>(out + 4 * w) = make_float4(v[0], v[1], v[2], v[3]);
    }
    for (long long g = 4 * n_words + first; g < total; g += stride) out[g] = cls_element(src, jobs, tab, H, W, mode, cval, st, cls_decode(g, H, W));
}

} // namespace

extern "C" {

int wsc_cls_train_batch(wsc_ctx *ctx, const uint8_t *images_dev, int B, const int32_t *size_hw_host, const int64_t *offset_host, int H,
                        int W, const double *affine_host, const int32_t *flags_host, int fill_mode, float cval, const float *sub3_host,
                        float div, float mul, float *x_dev) {
    WSC_CHECK(ctx && images_dev && size_hw_host && offset_host && affine_host && flags_host && sub3_host && x_dev, WSC_ERR_INVALID,
              "wsc_cls_train_batch: null argument");
    WSC_CHECK(B > 0 && B <= 65535, WSC_ERR_INVALID, "wsc_cls_train_batch: B=%d (1 .. 65535)", B);
    WSC_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, WSC_ERR_INVALID, "wsc_cls_train_batch: H=%d, W=%d (1 .. 32768)", H, W);
    WSC_CHECK(fill_mode == MODE_NEAREST || fill_mode == MODE_REFLECT || fill_mode == MODE_CONSTANT, WSC_ERR_INVALID,
              "wsc_cls_train_batch: fill_mode=%d (0 nearest, 1 reflect, 2 constant; scipy's 'wrap' is not supported)", fill_mode);
    WSC_CHECK(isfinite(cval) && isfinite(sub3_host[0]) && isfinite(sub3_host[1]) && isfinite(sub3_host[2]) && isfinite(div) && isfinite(mul),
              WSC_ERR_INVALID, "wsc_cls_train_batch: a standardisation constant or cval is not finite");
    WSC_CHECK(div != 0.0f, WSC_ERR_INVALID, "wsc_cls_train_batch: div = 0");
    for (int b = 0; b < B; ++b) {
        const int H0 = size_hw_host[2 * b], W0 = size_hw_host[2 * b + 1];
        WSC_CHECK(H0 > 0 && W0 > 0 && H0 <= 32768 && W0 <= 32768, WSC_ERR_INVALID, "wsc_cls_train_batch: sample %d has size %dx%d", b, H0, W0);
        WSC_CHECK(offset_host[b] >= 0, WSC_ERR_INVALID, "wsc_cls_train_batch: sample %d: negative offset", b);
        WSC_CHECK((flags_host[b] & ~(FLAG_WARP | FLAG_FLIP_COLS | FLAG_FLIP_ROWS)) == 0, WSC_ERR_INVALID,
                  "wsc_cls_train_batch: sample %d: flags=%d (bit 0 warp, bit 1 flip columns, bit 2 flip rows)", b, flags_host[b]);
        if (!(flags_host[b] & FLAG_WARP)) continue;
        const double *a = affine_host + 6 * b;
        for (int k = 0; k < 6; ++k)
            WSC_CHECK(isfinite(a[k]), WSC_ERR_INVALID, "wsc_cls_train_batch: sample %d: the warp's matrix or offset is not finite", b);
        // a coordinate is affine in (row, column): its extremes are at the corners.  Inside 2^20 pixels of the image the
        // integer conversions of the reflection are defined
        for (int k = 0; k < 2; ++k)
            for (int corner = 0; corner < 4; ++corner) {
                const double cc = a[4 + k] + (corner & 1 ? (double)(H - 1) : 0.0) * a[2 * k] + (corner & 2 ? (double)(W - 1) : 0.0) * a[2 * k + 1];
                const int n = k == 0 ? H : W;
                WSC_CHECK(isfinite(cc) && cc >= -MAX_REACH && cc <= (double)(n - 1) + MAX_REACH, WSC_ERR_INVALID,
                          "wsc_cls_train_batch: sample %d: the warp maps an output corner to %s %g, more than 2^20 pixels from the image", b,
                          k == 0 ? "row" : "column", cc);
            }
    }
    WSC_HIP(hipSetDevice(ctx->device));
    std::vector<ClsJob> jobs(B);
    std::vector<int32_t> tab;
    double src_bytes = 0.0;
    for (int b = 0; b < B; ++b) {
        ClsJob &j = jobs[b];
        j = ClsJob();
        j.src_off = offset_host[b];
        j.H0 = size_hw_host[2 * b];
        j.W0 = size_hw_host[2 * b + 1];
        j.ny_off = j.nx_off = -1;
        j.flags = flags_host[b];
        if (j.flags & FLAG_WARP)
            for (int k = 0; k < 6; ++k) j.a[k] = affine_host[6 * b + k];
        if (j.H0 != H || j.W0 != W) { // load_img resizes unless BOTH sides are right; an axis that keeps its size maps to itself
            j.ny_off = pil_add_nearest(tab, j.H0, H);
            j.nx_off = pil_add_nearest(tab, j.W0, W);
        }
        WSC_CHECK(tab.size() < TAB_MAX_INTS, WSC_ERR_INVALID, "wsc_cls_train_batch: sample %d: the tables outgrow %zu entries", b, TAB_MAX_INTS);
        src_bytes += 3.0 * j.H0 * j.W0;
    }
    WscStagedTable st(ctx);
    const size_t jo = st.add(jobs), to = st.add(tab);
    WSC_TRY(st.upload());
    ClsStd sd;
    sd.sub[0] = sub3_host[0];
    sd.sub[1] = sub3_host[1];
    sd.sub[2] = sub3_host[2];
    sd.div = div;
    sd.mul = mul;
    const long long total = (long long)B * 3 * H * W;
    const long long n_words = ((uintptr_t)x_dev & 15) == 0 ? total / 4 : 0;
    long long blocks = ((n_words > 0 ? n_words : total) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    {
        WscKernelTimer timer(ctx, WSC_K_POOL_MISC, src_bytes + 4.0 * (double)total);
        hipLaunchKernelGGL(cls_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, images_dev, st.at<const ClsJob>(jo),
                           st.at<const int>(to), H, W, fill_mode, cval, sd, n_words, total, x_dev);
        WSC_HIP(hipGetLastError());
    }
    st.release();
    return WSC_OK;
}

} // extern "C"
