// seg_batch.hip -- the inputs of a SEC / DSRG training step and the ground truth of a validation batch (03a_sec-dsrg) on the device:
//   wsc_seg_train_batch   Model.next_batch's m_train / get_data (model.py:229-252) with image_preprocess (:318-331): decoded uint8
//                         images and the sparse (class, row, col) cue lists of localization_cues.pickle in, the network's input,
//                         the dense 0/1 cue tensor and the label vector out
//   wsc_seg_gt_index_tf   m_val's ground truth (model.py:254-270, image_preprocess :338-342): TF 1.x resize_nearest_neighbor
//                         (align_corners=False), then the class test of eval_miou (:701, :709-714) -> uint8 class indices
// The image part IS wsc_seg_preprocess_u8 (seg_chain.hip), called as it stands: the same kernel, the same bits.
//
// seg_cues_kernel: a workgroup owns SLICE consecutive floats of one sample's [s][s][C] plane.  It walks that sample's list, sets
// the bits of the entries that fall into its slice in an LDS bitmask (ds_or: duplicates are idempotent), synchronises, and writes
// its slice as 0.0 / 1.0 -- every output element exactly once, 16-byte stores between a scalar head and tail that bring the
// address to the 16-byte grid (a plane of s*s*C floats need not be a multiple of four).  No memset, no global atomic.  The
// workgroups of slice 0 also write the sample's label row through one LDS word.
//
// The nearest rule is tf_tap's scale and product in float32 (tf_resize.h): src = min((int)floorf((float)dst * (in / out)), in - 1).
// An index computed in integers or in double differs from it (39 -> 33 at 11, 77 -> 33 at 27, 6 -> 321 at 107).  This file is
// compiled with -ffp-contract=off, as that header demands.
#include "common.h"
#include "tf_resize.h"

#include <limits.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int SLICE = 4096;            // floats of a plane per workgroup: 16 KB of stores, 512 B of bitmask
constexpr int SLICE_WORDS = SLICE / 32;
constexpr int SEG_MAX_SEED_PIXELS = 8192; // s * s

struct CueJob {
    long long cue_at; // int index of the sample's [3][n] block in the list table
    int n;            // entries
    int lab_at, n_lab; // int index and length of the sample's label list
};

// cue_tab: per sample [3][n] (class, row, col); cues: [B][s*s*C]; labels: [B][C]
__global__ __launch_bounds__(256) void seg_cues_kernel(const int *__restrict__ cue_tab, const int *__restrict__ lab_tab,
                                                       const CueJob *__restrict__ jobs, int s, int C, float *__restrict__ cues,
                                                       float *__restrict__ labels) {
    __shared__ unsigned mask[SLICE_WORDS];
    __shared__ unsigned lab_mask;
    const CueJob job = jobs[blockIdx.y];
    const int P = s * s * C; // <= 8192 * 32
    const int lo = blockIdx.x * SLICE, len = min(SLICE, P - lo);
    for (int k = threadIdx.x; k < SLICE_WORDS; k += blockDim.x) mask[k] = 0u;
    if (threadIdx.x == 0) lab_mask = 1u; // label[0] = 1.0
    __syncthreads();
    const int *cls = cue_tab + job.cue_at, *row = cls + job.n, *col = row + job.n;
    for (int k = threadIdx.x; k < job.n; k += blockDim.x) {
        const int r = (row[k] * s + col[k]) * C + cls[k] - lo; // (the entries were checked on the host)
        if (r >= 0 && r < len) atomicOr(&mask[r >> 5], 1u << (r & 31));
    }
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < job.n_lab; k += blockDim.x) atomicOr(&lab_mask, 1u << lab_tab[job.lab_at + k]);
    __syncthreads();
    auto bit = [&](int r) { return (float)((mask[r >> 5] >> (r & 31)) & 1u); };
    float *dst = cues + (long long)blockIdx.y * P + lo;
    const int head = min((int)((4u - (unsigned)(((uintptr_t)dst >> 2) & 3u)) & 3u), len);
    const int nvec = (len - head) >> 2, tail = head + 4 * nvec;
    if ((int)threadIdx.x < head) dst[threadIdx.x] = bit(threadIdx.x);
    for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
        const int r = head + 4 * v;
        f32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = bit(r + k);
        *reinterpret_cast<f32x4_t *>(dst + r) = o;
    }
    if ((int)threadIdx.x < len - tail) dst[tail + threadIdx.x] = bit(tail + threadIdx.x);
    if (blockIdx.x == 0 && (int)threadIdx.x < C) labels[(long long)blockIdx.y * C + threadIdx.x] = (float)((lab_mask >> threadIdx.x) & 1u);
}

struct GtJob {
    long long src_off; // byte offset of the ground truth's [h][w][channels] block
    int h, w;
};

// gt: packed uint8 blocks; colours: [n_class][3] or NULL; out: uint8 [B][OH][OW]
__global__ __launch_bounds__(256) void seg_gt_index_kernel(const uint8_t *__restrict__ gt, const GtJob *__restrict__ jobs, int channels,
                                                           const uint8_t *__restrict__ colours, int n_class, int OH, int OW,
                                                           uint8_t *__restrict__ out) {
    const GtJob job = jobs[blockIdx.y];
    const long long n = (long long)OH * OW;
    const float sy = (float)job.h / (float)OH, sx = (float)job.w / (float)OW;
    const uint8_t *src = gt + job.src_off;
    uint8_t *dst = out + (long long)blockIdx.y * n;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int Y = (int)(p / OW), X = (int)(p - (long long)Y * OW);
        int y0, y1, x0, x1;
        float ty, tx;
        tf_tap(Y, sy, job.h, y0, y1, ty); // y0 = min((int)floorf((float)Y * sy), h - 1): the nearest rule
        tf_tap(X, sx, job.w, x0, x1, tx);
        const uint8_t *px = src + ((long long)y0 * job.w + x0) * channels;
        int k;
        if (colours) {
            for (k = 0; k < n_class; ++k)
                if (px[0] == colours[3 * k] && px[1] == colours[3 * k + 1] && px[2] == colours[3 * k + 2]) break;
        } else {
            k = px[0] < n_class ? px[0] : n_class;
        }
        dst[p] = (uint8_t)k;
    }
}

// a ragged int32 table's offsets [B + 1]: not negative, not decreasing
const char *check_offsets(const int32_t *off, int B, int *bad) {
    if (off[0] < 0) {
        *bad = 0;
        return "negative";
    }
    for (int b = 0; b < B; ++b)
        if (off[b + 1] < off[b]) {
            *bad = b;
            return "decreasing";
        }
    return nullptr;
}

} // namespace

extern "C" {

int wsc_seg_train_batch(wsc_ctx *ctx, const uint8_t *img_dev, int B, const int32_t *src_hw_host, const int64_t *src_off_host,
                        const int32_t *cues_host, const int32_t *cue_off_host, const int32_t *labels_host,
                        const int32_t *label_off_host, const float *mean_bgr_host, int H, int W, int s, int C, float *x_dev,
                        float *cues_dev, float *labels_dev) {
    WSC_CHECK(ctx && img_dev && src_hw_host && src_off_host && cues_host && cue_off_host && labels_host && label_off_host &&
                  mean_bgr_host && x_dev && cues_dev && labels_dev,
              WSC_ERR_INVALID, "wsc_seg_train_batch: null argument");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_seg_train_batch: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(C >= 1 && C <= SEG_MAX_C, WSC_ERR_INVALID, "wsc_seg_train_batch: C=%d (1 <= C <= %d)", C, SEG_MAX_C);
    WSC_CHECK(s >= 1 && (long long)s * s <= SEG_MAX_SEED_PIXELS, WSC_ERR_INVALID, "wsc_seg_train_batch: seed size s=%d (s >= 1, s * s <= %d)", s,
              SEG_MAX_SEED_PIXELS);
    WSC_CHECK(H >= 1 && W >= 1 && (long long)H * W <= INT_MAX, WSC_ERR_INVALID,
              "wsc_seg_train_batch: target H=%d W=%d (both >= 1, H * W within int32)", H, W);
    int bad = 0;
    const char *why = check_offsets(cue_off_host, B, &bad);
    WSC_CHECK(!why, WSC_ERR_INVALID, "wsc_seg_train_batch: sample %d: %s cue offset", bad, why);
    why = check_offsets(label_off_host, B, &bad);
    WSC_CHECK(!why, WSC_ERR_INVALID, "wsc_seg_train_batch: sample %d: %s label offset", bad, why);
    WSC_CHECK(cue_off_host[B] <= INT_MAX / 3, WSC_ERR_INVALID, "wsc_seg_train_batch: %d cue entries (3 ints each, within int32)", cue_off_host[B]);
    std::vector<CueJob> jobs(B);
    for (int b = 0; b < B; ++b) {
        const int h = src_hw_host[2 * b], w = src_hw_host[2 * b + 1];
        WSC_CHECK(h >= 1 && w >= 1 && (long long)h * w <= INT_MAX, WSC_ERR_INVALID,
                  "wsc_seg_train_batch: sample %d: image %d x %d (both >= 1, h * w within int32)", b, h, w);
        WSC_CHECK(src_off_host[b] >= 0, WSC_ERR_INVALID, "wsc_seg_train_batch: sample %d: image offset %lld is negative", b,
                  (long long)src_off_host[b]);
        CueJob &j = jobs[b];
        j.cue_at = 3LL * cue_off_host[b];
        j.n = cue_off_host[b + 1] - cue_off_host[b];
        j.lab_at = label_off_host[b];
        j.n_lab = label_off_host[b + 1] - label_off_host[b];
        const int32_t *cls = cues_host + j.cue_at, *row = cls + j.n, *col = row + j.n;
        for (int k = 0; k < j.n; ++k) {
            WSC_CHECK(cls[k] >= 0 && cls[k] < C, WSC_ERR_INVALID, "wsc_seg_train_batch: sample %d: cue %d has class %d (0 <= class < %d)", b, k,
                      cls[k], C);
            WSC_CHECK(row[k] >= 0 && row[k] < s && col[k] >= 0 && col[k] < s, WSC_ERR_INVALID,
                      "wsc_seg_train_batch: sample %d: cue %d at row %d, column %d (0 <= both < %d)", b, k, row[k], col[k], s);
        }
        for (int k = 0; k < j.n_lab; ++k)
            WSC_CHECK(labels_host[j.lab_at + k] >= 0 && labels_host[j.lab_at + k] < C, WSC_ERR_INVALID,
                      "wsc_seg_train_batch: sample %d: label %d is class %d (0 <= class < %d)", b, k, labels_host[j.lab_at + k], C);
    }
    // the image part: the entry point itself (its own checks repeat the ones above and cannot fail after them)
    WSC_TRY(wsc_seg_preprocess_u8(ctx, img_dev, B, src_hw_host, src_off_host, mean_bgr_host, H, W, x_dev));
    WscStagedTable tab(ctx);
    const size_t jo = tab.add(jobs.data(), jobs.size() * sizeof(CueJob));
    const size_t co = tab.add(cues_host, 3 * (size_t)cue_off_host[B] * sizeof(int32_t));
    const size_t lo = tab.add(labels_host, (size_t)label_off_host[B] * sizeof(int32_t));
    WSC_TRY(tab.upload());
    const int P = s * s * C;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, 12.0 * cue_off_host[B] + 4.0 * B * ((double)P + C));
    hipLaunchKernelGGL(seg_cues_kernel, dim3((unsigned)((P + SLICE - 1) / SLICE), (unsigned)B), dim3(256), 0, ctx->stream,
                       tab.at<const int>(co), tab.at<const int>(lo), tab.at<const CueJob>(jo), s, C, cues_dev, labels_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

int wsc_seg_gt_index_tf(wsc_ctx *ctx, const uint8_t *gt_dev, int B, const int32_t *src_hw_host, const int64_t *src_off_host,
                        int channels, const uint8_t *colours_host, int n_class, int OH, int OW, uint8_t *index_dev) {
    WSC_CHECK(ctx && gt_dev && src_hw_host && src_off_host && index_dev, WSC_ERR_INVALID, "wsc_seg_gt_index_tf: null argument");
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_seg_gt_index_tf: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(n_class >= 1 && n_class <= SEG_MAX_C, WSC_ERR_INVALID, "wsc_seg_gt_index_tf: n_class=%d (1 <= n_class <= %d)", n_class, SEG_MAX_C);
    WSC_CHECK(channels == 1 || channels == 3, WSC_ERR_INVALID, "wsc_seg_gt_index_tf: channels=%d (1 or 3)", channels);
    WSC_CHECK(!colours_host || channels == 3, WSC_ERR_INVALID, "wsc_seg_gt_index_tf: a colour table needs 3 channels, not %d", channels);
    WSC_CHECK(OH >= 1 && OW >= 1 && (long long)OH * OW <= INT_MAX, WSC_ERR_INVALID,
              "wsc_seg_gt_index_tf: target OH=%d OW=%d (both >= 1, OH * OW within int32)", OH, OW);
    std::vector<GtJob> jobs(B);
    double src_bytes = 0;
    for (int b = 0; b < B; ++b) {
        GtJob &j = jobs[b];
        j.h = src_hw_host[2 * b];
        j.w = src_hw_host[2 * b + 1];
        j.src_off = src_off_host[b];
        WSC_CHECK(j.h >= 1 && j.w >= 1 && (long long)j.h * j.w <= INT_MAX, WSC_ERR_INVALID,
                  "wsc_seg_gt_index_tf: sample %d: ground truth %d x %d (both >= 1, h * w within int32)", b, j.h, j.w);
        WSC_CHECK(j.src_off >= 0, WSC_ERR_INVALID, "wsc_seg_gt_index_tf: sample %d: offset %lld is negative", b, (long long)j.src_off);
        src_bytes += (double)channels * j.h * j.w;
    }
    WSC_HIP(hipSetDevice(ctx->device));
    WscStagedTable tab(ctx);
    const size_t jo = tab.add(jobs);
    const size_t co = tab.add(colours_host, colours_host ? 3 * (size_t)n_class : 0);
    WSC_TRY(tab.upload());
    const long long npix = (long long)OH * OW;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, src_bytes + (double)B * (double)npix);
    hipLaunchKernelGGL(seg_gt_index_kernel, dim3((unsigned)std::min<long long>((npix + 255) / 256, 1024), (unsigned)B), dim3(256), 0,
                       ctx->stream, gt_dev, tab.at<const GtJob>(jo), channels, colours_host ? tab.at<const uint8_t>(co) : nullptr, n_class,
                       OH, OW, index_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

} // extern "C"
