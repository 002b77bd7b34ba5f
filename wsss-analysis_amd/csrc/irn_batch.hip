// irn_batch.hip -- the IRNet training-sample transform on the device: decoded uint8 images and IR labels in, one training batch out.
//
// Reference (host, PIL / numpy, per sample): 03b_irn/voc12/dataloader.py:270-321 (VOC12AffinityDataset.__getitem__; the ADP and
// DeepGlobe twins adp/dataloader.py:270-321, deepglobe/dataloader.py:257-308) --
//   imutils.random_scale((img, label), order=(3, 0))   PIL bicubic on the image, PIL nearest on the label
//   TorchvisionResize (vgg16 / m7: outsize)            float64 bilinear of image AND label
//   TorchvisionNormalize, random_lr_flip, random_crop((img, label), S, (0, 255)), HWC_to_CHW
//   imutils.pil_rescale(label, 0.25, 0)                the label at the resolution of the head outputs
// Several milliseconds of PIL and numpy per sample on the host and 3 MB of float32 per sample over PCIe; here the decoded
// bytes travel and two HBM-bound integer kernels do the rest.
//
// PIL's resample (Resample.c, 8 bits per channel), restated: per axis, horizontal pass first, uint8 intermediate, a pass whose
// axis keeps its size skipped;
//   scale = in / out; fs = max(scale, 1); support = 2 fs; per output i: center = (i + 0.5) scale,
//   xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in) - xmin,
//   w[k] = bicubic((k + xmin - center + 0.5) / fs) normalised by their sum in index order,
//   coef[k] = (int)(w[k] 2^22 -+ 0.5), out = clamp((2^21 + sum coef[k] pixel[xmin + k]) >> 22, 0, 255).
// PIL's nearest (Geometry.c, ImagingScaleAffine): a = in / out, v = a / 2, per index idx = (int)v, v += a (the running sum).
// The tables are built on the HOST, in double, in PIL's order of operations, and travel with the job records in one staged
// table; the kernels are pure integer arithmetic (stage 2's float64 bilinear aside), so no device division can move a
// coefficient.  The numpy restatement tests/irn_batch_ref.py is pinned against Image.resize itself; the kernels against it,
// every byte and bit.
//
// This file is compiled with -ffp-contract=off: stage 2's interpolation is the sequence of float64 products and sums of
// input.hip's msf_input_kernel, the normalisation one fp32 subtract and one fp32 divide.
#include "common.h"
#include "pil_nearest.h"

#include <math.h>

#include <vector>

namespace {

constexpr int PIL_BITS = 22; // PRECISION_BITS of Resample.c

struct BatchJob {
    long long src_off, lab_off; // bytes of the sample's image / label in their packed buffers
    long long tmp_off;          // bytes of pass 1's rows in the temporary
    long long out_off;          // wsc_pil_resize_u8: bytes of the result in out_dev
    int H0, W0;                 // the source
    int sh, sw;                 // the resized image
    int flip, cont_top, cont_left, img_top, img_left, ch, cw;
    int row0, nrows;            // the source rows pass 1 resamples: [row0, row0 + nrows)
    int h_off, h_k;             // horizontal table: [sw] xmin, [sw] n, [sw][h_k] coefficients; h_off < 0: the width is kept
    int v_first, v_rows;        // the output rows the vertical table covers: [v_first, v_first + v_rows)
    int v_off, v_k;             // vertical table: [v_rows] ymin, [v_rows] n, [v_rows][v_k] coefficients; v_off < 0: height kept
    int nx_off, ny_off;         // nearest tables [sw] / [sh]: resized column / row -> source; < 0: the size is kept
};

__device__ __forceinline__ int pil_dot(const uint8_t *__restrict__ p, long long stride, const int *__restrict__ coef, int n) {
    int ss = 1 << (PIL_BITS - 1);
    for (int k = 0; k < n; ++k) ss += coef[k] * (int)p[(long long)k * stride];
    ss >>= PIL_BITS; // arithmetic
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// the rows the vertical taps read: pass 1's (pitch sw * C, first row row0), or the source itself where the width is kept
__device__ __forceinline__ const uint8_t *job_rows(const BatchJob &job, const uint8_t *src, const uint8_t *tmp, int &row0) {
    if (job.h_off >= 0) {
        row0 = job.row0;
        return tmp + job.tmp_off;
    }
    row0 = 0;
    return src + job.src_off;
}

// value (y, rem) of the resized image, rem = x * C + c
__device__ __forceinline__ int pil_vertical(const BatchJob &job, const uint8_t *rows, int row0, long long pitch, const int *__restrict__ tab,
                                            int y, int rem) {
    if (job.v_off < 0) return rows[(long long)(y - row0) * pitch + rem];
    const int j = y - job.v_first;
    const int *t = tab + job.v_off;
    const int ymin = t[j], n = t[job.v_rows + j];
    return pil_dot(rows + (long long)(ymin - row0) * pitch + rem, pitch, t + 2 * job.v_rows + (long long)j * job.v_k, n);
}

// Pass 1: tmp[r][x][c] = the horizontal resample of source row row0 + r; threads run along sw * C
__global__ __launch_bounds__(256) void pil_hpass_kernel(const uint8_t *__restrict__ src, const BatchJob *__restrict__ jobs,
                                                        const int *__restrict__ tab, int C, uint8_t *__restrict__ tmp) {
    const BatchJob job = jobs[blockIdx.y];
    if (job.h_off < 0) return;
    const int pitch = job.sw * C;
    const long long n = (long long)job.nrows * pitch;
    const int *t = tab + job.h_off;
    const uint8_t *im = src + job.src_off;
    uint8_t *dst = tmp + job.tmp_off;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(e / pitch), rem = (int)(e - (long long)r * pitch);
        const int x = rem / C, c = rem - x * C;
        const int xmin = t[x], cnt = t[job.sw + x];
        dst[e] = (uint8_t)pil_dot(im + ((long long)(job.row0 + r) * job.W0 + xmin) * C + c, C, t + 2 * job.sw + (long long)x * job.h_k, cnt);
    }
}

// The plain vertical pass of wsc_pil_resize_u8: out[y][x][c], uint8
__global__ __launch_bounds__(256) void pil_vpass_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ tmp,
                                                        const BatchJob *__restrict__ jobs, const int *__restrict__ tab, int C,
                                                        uint8_t *__restrict__ out) {
    const BatchJob job = jobs[blockIdx.y];
    int row0;
    const uint8_t *rows = job_rows(job, src, tmp, row0);
    const int pitch = job.sw * C;
    const long long n = (long long)job.sh * pitch;
    uint8_t *dst = out + job.out_off;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(e / pitch), rem = (int)(e - (long long)y * pitch);
        dst[e] = (uint8_t)pil_vertical(job, rows, row0, pitch, tab, y, rem);
    }
}

// Image.resize(NEAREST): out[y][x][c] = src[ny[y]][nx[x]][c]
__global__ __launch_bounds__(256) void pil_nearest_kernel(const uint8_t *__restrict__ src, const BatchJob *__restrict__ jobs,
                                                          const int *__restrict__ tab, int C, uint8_t *__restrict__ out) {
    const BatchJob job = jobs[blockIdx.y];
    const int pitch = job.sw * C;
    const long long n = (long long)job.sh * pitch;
    const uint8_t *im = src + job.src_off;
    uint8_t *dst = out + job.out_off;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(e / pitch), rem = (int)(e - (long long)y * pitch);
        const int x = rem / C, c = rem - x * C;
        const int sy = job.ny_off < 0 ? y : tab[job.ny_off + y], sx = job.nx_off < 0 ? x : tab[job.nx_off + x];
        dst[e] = im[((long long)sy * job.W0 + sx) * C + c];
    }
}

// TorchvisionResize's float64 bilinear (cv2.resize INTER_LINEAR on a float64 array) at (yy, xx) of an OH x OW result: the
// expression of msf_input_kernel (input.hip), channel c of a C-channel uint8 source
__device__ __forceinline__ double bilinear_f64(const uint8_t *__restrict__ im, int H, int W, int C, int c, int yy, int xx, int OH, int OW) {
    if (H == OH && W == OW) return (double)im[((long long)yy * W + xx) * C + c];
    double fy = ((double)yy + 0.5) * (double)H / (double)OH - 0.5;
    double fx = ((double)xx + 0.5) * (double)W / (double)OW - 0.5;
    fy = fy < 0.0 ? 0.0 : (fy > (double)(H - 1) ? (double)(H - 1) : fy);
    fx = fx < 0.0 ? 0.0 : (fx > (double)(W - 1) ? (double)(W - 1) : fx);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const double wy = fy - (double)y0, wx = fx - (double)x0;
    const double a = (double)im[((long long)y0 * W + x0) * C + c], b = (double)im[((long long)y0 * W + x1) * C + c];
    const double d = (double)im[((long long)y1 * W + x0) * C + c], e = (double)im[((long long)y1 * W + x1) * C + c];
    const double top = a * (1.0 - wx) + b * wx;
    const double bot = d * (1.0 - wx) + e * wx;
    return top * (1.0 - wy) + bot * wy;
}

// (y, x) of the S x S container -> (iy, sx) of the resized, UNFLIPPED sample; false: padding
__device__ __forceinline__ bool crop_source(const BatchJob &job, int y, int x, int &iy, int &sx) {
    const int wy = y - job.cont_top, wx = x - job.cont_left;
    if (wy < 0 || wy >= job.ch || wx < 0 || wx >= job.cw) return false;
    iy = wy + job.img_top;
    const int ix = wx + job.img_left;
    sx = job.flip ? job.sw - 1 - ix : ix; // np.fliplr before the crop
    return true;
}

// the cropped label at (y, x) of the container: through the two nearest tables (stage 1), the truncated float64 bilinear
// (stage 2: np.uint8 of the float label) or as it is
__device__ __forceinline__ uint8_t crop_label(const BatchJob &job, const uint8_t *__restrict__ lab, const int *__restrict__ tab, int stage, int y,
                                              int x) {
    int iy, sx;
    if (!crop_source(job, y, x, iy, sx)) return 255;
    if (stage == 2) return (uint8_t)(int)bilinear_f64(lab, job.H0, job.W0, 1, 0, iy, sx, job.sh, job.sw);
    const int ly = job.ny_off < 0 ? iy : tab[job.ny_off + iy], lx = job.nx_off < 0 ? sx : tab[job.nx_off + sx];
    return lab[(long long)ly * job.W0 + lx];
}

// Pass 2, fused: one thread per (b, y, x) of the crop -- the vertical taps at the flipped, crop-shifted column, clip, normalise,
// the three CHW stores, the label, and on the reduced grid the reduced label
__global__ __launch_bounds__(256) void irn_batch_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ labels,
                                                        const uint8_t *__restrict__ tmp, const BatchJob *__restrict__ jobs,
                                                        const int *__restrict__ tab, int r_off, int S, int s, int stage, float m0, float m1,
                                                        float m2, float s0, float s1, float s2, int pre_div255, float *__restrict__ x_out,
                                                        uint8_t *__restrict__ label_out, uint8_t *__restrict__ reduced_out) {
    const BatchJob job = jobs[blockIdx.y];
    const int n = S * S;
    int row0;
    const uint8_t *rows = job_rows(job, src, tmp, row0);
    const uint8_t *lab = labels + job.lab_off;
    const long long pitch = (long long)job.sw * 3;
    float *xb = x_out + (long long)blockIdx.y * 3 * n;
    uint8_t *lb = label_out + (long long)blockIdx.y * n, *rb = reduced_out + (long long)blockIdx.y * s * s;
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = i / S, x = i - y * S;
        int iy, sx;
        if (crop_source(job, y, x, iy, sx)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float f;
                if (stage == 2) f = (float)bilinear_f64(src + job.src_off, job.H0, job.W0, 3, c, iy, sx, job.sh, job.sw);
                else f = (float)pil_vertical(job, rows, row0, pitch, tab, iy, sx * 3 + c);
                if (pre_div255) f = f / 255.0f;
                xb[(long long)c * n + i] = (f - mean[c]) / sd[c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) xb[(long long)c * n + i] = 0.0f;
        }
        lb[i] = crop_label(job, lab, tab, stage, y, x);
        if (y < s && x < s) rb[y * s + x] = crop_label(job, lab, tab, stage, tab[r_off + y], tab[r_off + x]);
    }
}

// ---- the host side: PIL's tables ------------------------------------------------------------------------------------------------
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// precompute_coeffs + normalize_coeffs_8bpc for the outputs [o0, o0 + cnt) of an axis in -> out, appended to tab as [cnt] xmin,
// [cnt] n, [cnt][*ksize] coefficients; -> the int32 index of the section; [*lo, *hi): the source indices the taps touch
int add_resample(std::vector<int32_t> &tab, int in, int out, int o0, int cnt, int *ksize, int *lo, int *hi) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const int K = (int)ceil(support) * 2 + 1;
    const size_t off = tab.size();
    tab.resize(off + (size_t)cnt * (2 + K), 0);
    std::vector<double> w(K);
    *lo = in;
    *hi = 0;
    for (int j = 0; j < cnt; ++j) {
        const double center = ((o0 + j) + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        int n = xmax - xmin;
        if (n > K) n = K; // (never: K bounds the window)
        double ww = 0.0;
        for (int k = 0; k < n; ++k) {
            w[k] = bicubic_filter((k + xmin - center + 0.5) * ss);
            ww += w[k];
        }
        int32_t *coef = tab.data() + off + 2 * (size_t)cnt + (size_t)j * K;
        for (int k = 0; k < n; ++k) {
            if (ww != 0.0) w[k] /= ww;
            coef[k] = w[k] < 0 ? (int)(-0.5 + w[k] * (1 << PIL_BITS)) : (int)(0.5 + w[k] * (1 << PIL_BITS));
        }
        tab[off + j] = xmin;
        tab[off + cnt + j] = n;
        if (xmin < *lo) *lo = xmin;
        if (xmin + n > *hi) *hi = xmin + n;
    }
    *ksize = K;
    return (int)off;
}

constexpr size_t TAB_MAX_INTS = (size_t)1 << 28; // int32 indices into the table

unsigned grid_x(long long n, int cap) {
    long long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

} // namespace

extern "C" {

int wsc_pil_resize_u8(wsc_ctx *ctx, const uint8_t *images_dev, int B, const int32_t *size_hw_host, const int64_t *offset_host,
                      const int32_t *out_hw_host, const int64_t *out_offset_host, int channels, int order, uint8_t *out_dev) {
    WSC_CHECK(ctx && images_dev && size_hw_host && offset_host && out_hw_host && out_offset_host && out_dev, WSC_ERR_INVALID,
              "wsc_pil_resize_u8: null argument");
    WSC_CHECK(B > 0 && B <= 65535, WSC_ERR_INVALID, "wsc_pil_resize_u8: B=%d (1 .. 65535)", B);
    WSC_CHECK(channels == 1 || channels == 3, WSC_ERR_INVALID, "wsc_pil_resize_u8: channels=%d (1 or 3)", channels);
    WSC_CHECK(order == 3 || order == 0, WSC_ERR_INVALID, "wsc_pil_resize_u8: order=%d (3 = bicubic, 0 = nearest)", order);
    for (int b = 0; b < B; ++b) {
        WSC_CHECK(size_hw_host[2 * b] > 0 && size_hw_host[2 * b + 1] > 0 && out_hw_host[2 * b] > 0 && out_hw_host[2 * b + 1] > 0 &&
                      size_hw_host[2 * b] <= 32768 && size_hw_host[2 * b + 1] <= 32768 && out_hw_host[2 * b] <= 32768 &&
                      out_hw_host[2 * b + 1] <= 32768,
                  WSC_ERR_INVALID, "wsc_pil_resize_u8: image %d: %dx%d -> %dx%d (every side 1 .. 32768)", b, size_hw_host[2 * b],
                  size_hw_host[2 * b + 1], out_hw_host[2 * b], out_hw_host[2 * b + 1]);
        WSC_CHECK(offset_host[b] >= 0 && out_offset_host[b] >= 0, WSC_ERR_INVALID, "wsc_pil_resize_u8: image %d: negative offset", b);
    }
    WSC_HIP(hipSetDevice(ctx->device));
    std::vector<BatchJob> jobs(B);
    std::vector<int32_t> tab;
    long long tmp_bytes = 0, max_h = 1, max_o = 1;
    bool any_h = false;
    for (int b = 0; b < B; ++b) {
        BatchJob &j = jobs[b];
        j = BatchJob();
        j.src_off = offset_host[b];
        j.out_off = out_offset_host[b];
        j.H0 = size_hw_host[2 * b];
        j.W0 = size_hw_host[2 * b + 1];
        j.sh = out_hw_host[2 * b];
        j.sw = out_hw_host[2 * b + 1];
        j.h_off = j.v_off = j.nx_off = j.ny_off = -1;
        j.row0 = 0;
        j.nrows = j.H0;
        if (order == 0) {
            j.ny_off = pil_add_nearest(tab, j.H0, j.sh);
            j.nx_off = pil_add_nearest(tab, j.W0, j.sw);
        } else {
            if (j.sh != j.H0) {
                int lo, hi;
                j.v_first = 0;
                j.v_rows = j.sh;
                j.v_off = add_resample(tab, j.H0, j.sh, 0, j.sh, &j.v_k, &lo, &hi);
                j.row0 = lo;
                j.nrows = hi - lo;
            }
            if (j.sw != j.W0) {
                int lo, hi;
                j.h_off = add_resample(tab, j.W0, j.sw, 0, j.sw, &j.h_k, &lo, &hi);
                j.tmp_off = tmp_bytes;
                tmp_bytes += ((long long)j.nrows * j.sw * channels + 15) / 16 * 16;
                any_h = true;
                if ((long long)j.nrows * j.sw * channels > max_h) max_h = (long long)j.nrows * j.sw * channels;
            }
        }
        WSC_CHECK(tab.size() < TAB_MAX_INTS, WSC_ERR_INVALID, "wsc_pil_resize_u8: image %d: the tables outgrow %zu entries", b, TAB_MAX_INTS);
        if ((long long)j.sh * j.sw * channels > max_o) max_o = (long long)j.sh * j.sw * channels;
    }
    WscStagedTable st(ctx);
    const size_t jo = st.add(jobs), to = st.add(tab);
    WSC_TRY(st.upload());
    void *tmp = nullptr;
    if (any_h) WSC_TRY(wsc_ctx_cached_alloc(ctx, (size_t)tmp_bytes, &tmp));
    WscCachedGuard tmp_guard(ctx, tmp);
    const BatchJob *jd = st.at<const BatchJob>(jo);
    const int *td = st.at<const int>(to);
    if (order == 0) {
        WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 2.0 * B * (double)max_o);
        hipLaunchKernelGGL(pil_nearest_kernel, dim3(grid_x(max_o, 512), (unsigned)B), dim3(256), 0, ctx->stream, images_dev, jd, td, channels,
                           out_dev);
        WSC_HIP(hipGetLastError());
    } else {
        if (any_h) {
            WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 2.0 * (double)tmp_bytes);
            hipLaunchKernelGGL(pil_hpass_kernel, dim3(grid_x(max_h, 512), (unsigned)B), dim3(256), 0, ctx->stream, images_dev, jd, td, channels,
                               (uint8_t *)tmp);
            WSC_HIP(hipGetLastError());
        }
        WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 2.0 * B * (double)max_o);
        hipLaunchKernelGGL(pil_vpass_kernel, dim3(grid_x(max_o, 512), (unsigned)B), dim3(256), 0, ctx->stream, images_dev, (const uint8_t *)tmp,
                           jd, td, channels, out_dev);
        WSC_HIP(hipGetLastError());
    }
    tmp_guard.free_now(); // stream-ordered reuse
    st.release();
    return WSC_OK;
}

int wsc_irn_train_batch(wsc_ctx *ctx, const uint8_t *images_dev, const uint8_t *labels_dev, int B, const int32_t *size_hw_host,
                        const int64_t *image_offset_host, const int64_t *label_offset_host, const int32_t *params_host, int S,
                        const float *mean3_host, const float *std3_host, int pre_div255, int stage, float *x_dev, uint8_t *label_dev,
                        uint8_t *reduced_dev) {
    WSC_CHECK(ctx && images_dev && labels_dev && size_hw_host && image_offset_host && label_offset_host && params_host && mean3_host &&
                  std3_host && x_dev && label_dev && reduced_dev,
              WSC_ERR_INVALID, "wsc_irn_train_batch: null argument");
    WSC_CHECK(B > 0 && B <= 65535, WSC_ERR_INVALID, "wsc_irn_train_batch: B=%d (1 .. 65535)", B);
    WSC_CHECK(S >= 2 && S <= 8192, WSC_ERR_INVALID, "wsc_irn_train_batch: S=%d (2 .. 8192)", S);
    WSC_CHECK(stage >= 0 && stage <= 2, WSC_ERR_INVALID, "wsc_irn_train_batch: stage=%d (0 none, 1 PIL rescale, 2 TorchvisionResize)", stage);
    const int s = (int)nearbyint((double)S * 0.25); // np.round: half to even
    WSC_CHECK(s >= 1, WSC_ERR_INVALID, "wsc_irn_train_batch: S=%d leaves no reduced label", S);
    for (int b = 0; b < B; ++b) {
        const int32_t *p = params_host + 9 * b;
        const int H0 = size_hw_host[2 * b], W0 = size_hw_host[2 * b + 1], sh = p[0], sw = p[1];
        WSC_CHECK(H0 > 0 && W0 > 0 && H0 <= 32768 && W0 <= 32768, WSC_ERR_INVALID, "wsc_irn_train_batch: sample %d has size %dx%d", b, H0, W0);
        WSC_CHECK(sh > 0 && sw > 0 && sh <= 32768 && sw <= 32768, WSC_ERR_INVALID, "wsc_irn_train_batch: sample %d: resized to %dx%d", b, sh, sw);
        WSC_CHECK(image_offset_host[b] >= 0 && label_offset_host[b] >= 0, WSC_ERR_INVALID, "wsc_irn_train_batch: sample %d: negative offset", b);
        WSC_CHECK(stage != 0 || (sh == H0 && sw == W0), WSC_ERR_INVALID,
                  "wsc_irn_train_batch: sample %d is %dx%d, not %dx%d, and stage 0 does not resize", b, H0, W0, sh, sw);
        WSC_CHECK(p[2] == 0 || p[2] == 1, WSC_ERR_INVALID, "wsc_irn_train_batch: sample %d: flip=%d", b, p[2]);
        const int ct = p[3], cl = p[4], it = p[5], il = p[6], ch = p[7], cw = p[8];
        WSC_CHECK(ch >= 1 && cw >= 1 && it >= 0 && il >= 0 && it <= sh - ch && il <= sw - cw, WSC_ERR_INVALID,
                  "wsc_irn_train_batch: sample %d: window rows %d+%d, columns %d+%d leave the %dx%d image", b, it, ch, il, cw, sh, sw);
        WSC_CHECK(ct >= 0 && cl >= 0 && ct <= S - ch && cl <= S - cw, WSC_ERR_INVALID,
                  "wsc_irn_train_batch: sample %d: window rows %d+%d, columns %d+%d leave the %dx%d container", b, ct, ch, cl, cw, S, S);
    }
    WSC_HIP(hipSetDevice(ctx->device));
    std::vector<BatchJob> jobs(B);
    std::vector<int32_t> tab;
    const int r_off = pil_add_nearest(tab, S, s);
    long long tmp_bytes = 0, max_h = 1;
    bool any_h = false;
    for (int b = 0; b < B; ++b) {
        const int32_t *p = params_host + 9 * b;
        BatchJob &j = jobs[b];
        j = BatchJob();
        j.src_off = image_offset_host[b];
        j.lab_off = label_offset_host[b];
        j.H0 = size_hw_host[2 * b];
        j.W0 = size_hw_host[2 * b + 1];
        j.sh = p[0]; j.sw = p[1]; j.flip = p[2];
        j.cont_top = p[3]; j.cont_left = p[4]; j.img_top = p[5]; j.img_left = p[6]; j.ch = p[7]; j.cw = p[8];
        j.h_off = j.v_off = j.nx_off = j.ny_off = -1;
        j.row0 = j.img_top;
        j.nrows = j.ch;
        if (stage == 1 && (j.sh != j.H0 || j.sw != j.W0)) {
            j.ny_off = pil_add_nearest(tab, j.H0, j.sh);
            j.nx_off = pil_add_nearest(tab, j.W0, j.sw);
            if (j.sh != j.H0) { // the vertical taps of the window's rows, and the source rows they touch
                int lo, hi;
                j.v_first = j.img_top;
                j.v_rows = j.ch;
                j.v_off = add_resample(tab, j.H0, j.sh, j.img_top, j.ch, &j.v_k, &lo, &hi);
                j.row0 = lo;
                j.nrows = hi - lo;
            }
            if (j.sw != j.W0) {
                int lo, hi;
                j.h_off = add_resample(tab, j.W0, j.sw, 0, j.sw, &j.h_k, &lo, &hi);
                j.tmp_off = tmp_bytes;
                tmp_bytes += ((long long)j.nrows * j.sw * 3 + 15) / 16 * 16;
                any_h = true;
                if ((long long)j.nrows * j.sw * 3 > max_h) max_h = (long long)j.nrows * j.sw * 3;
            }
        }
        WSC_CHECK(tab.size() < TAB_MAX_INTS, WSC_ERR_INVALID, "wsc_irn_train_batch: sample %d: the tables outgrow %zu entries", b, TAB_MAX_INTS);
    }
    WscStagedTable st(ctx);
    const size_t jo = st.add(jobs), to = st.add(tab);
    WSC_TRY(st.upload());
    void *tmp = nullptr;
    if (any_h) WSC_TRY(wsc_ctx_cached_alloc(ctx, (size_t)tmp_bytes, &tmp));
    WscCachedGuard tmp_guard(ctx, tmp);
    const BatchJob *jd = st.at<const BatchJob>(jo);
    const int *td = st.at<const int>(to);
    if (any_h) {
        WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 2.0 * (double)tmp_bytes);
        hipLaunchKernelGGL(pil_hpass_kernel, dim3(grid_x(max_h, 512), (unsigned)B), dim3(256), 0, ctx->stream, images_dev, jd, td, 3,
                           (uint8_t *)tmp);
        WSC_HIP(hipGetLastError());
    }
    {
        WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * S * S * (3 * 4 + 1 + 3 * 3));
        hipLaunchKernelGGL(irn_batch_kernel, dim3(grid_x((long long)S * S, 1024), (unsigned)B), dim3(256), 0, ctx->stream, images_dev,
                           labels_dev, (const uint8_t *)tmp, jd, td, r_off, S, s, stage, mean3_host[0], mean3_host[1], mean3_host[2],
                           std3_host[0], std3_host[1], std3_host[2], pre_div255, x_dev, label_dev, reduced_dev);
        WSC_HIP(hipGetLastError());
    }
    tmp_guard.free_now(); // stream-ordered reuse
    st.release();
    return WSC_OK;
}

} // extern "C"
