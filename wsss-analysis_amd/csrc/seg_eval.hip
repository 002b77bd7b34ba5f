// seg_eval.hip -- the glue around the dense CRF in the SEC / DSRG prediction loop (03a_sec-dsrg/model.py:665-719, eval_miou with
// is_eval=True, called from predict :542-586).
//
//   seg_unary_nhwc_kernel      model.py:686,689: cv2.resize of the network's (h, w, C) softmax to the ground truth's size and the
//                              unary -log(.) of lib.crf.crf_inference(use_log=True), written class-major for wsc_crf_v_inference
//   seg_resize_argmax_kernel   model.py:695,699 (DeepGlobe): cv2.resize of the CRF marginals to the ground truth's size and
//                              np.argmax over the classes; the resized marginals are never written
// Both take a ragged batch as one launch: grid.y = image, descriptors in a small device table (as cam_tail.hip's kernels).
// One thread owns one output pixel: it forms its four tap indices and weights once and walks the classes.  The class-major
// stores (and the label stores) are one dword per lane, consecutive across a wave; the NHWC taps are C contiguous floats each,
// read 16 bytes at a time where C and the block's alignment allow.  Both kernels are bound by their stores when they upsample
// (the source stays in cache) and by the tap reads when they shrink.
// The sampler is bilerp.h's -- src_index with separate fp32 scales h / H and w / W, the fused multiply-adds spelled out -- so a
// resized value has the bits wsc_bilinear_resize (bilinear_kernel) gives for that class plane, and equal sizes give weights of
// exactly 1 and 0: the map passes through unchanged.  csrc/hsn.hip records that this half-pixel, clamped rule is cv2's
// INTER_LINEAR rule; cv2 is absent offline, so parity with cv2's own float arithmetic is unpinned.
#include "common.h"
#include "bilerp.h"

#include <limits.h>

#include <algorithm>

namespace {

struct SegJob {
    long long src_off; // float offset of the image's source block
    long long dst_off; // element offset of the image's output block
    int h, w, H, W;    // source and output size
};

// prob: image b's [h][w][C] block at src_off; unary: its [C][H*W] block at dst_off.  VEC4: C % 4 == 0 and every block starts on
// a 16-byte boundary.
template <bool VEC4>
__global__ __launch_bounds__(256) void seg_unary_nhwc_kernel(const float *__restrict__ prob, const SegJob *__restrict__ jobs, int C,
                                                             float *__restrict__ unary) {
    const SegJob job = jobs[blockIdx.y];
    const long long n = (long long)job.H * job.W;
    const float sh = (float)job.h / (float)job.H, sw = (float)job.w / (float)job.W;
    const float *src = prob + job.src_off;
    float *dst = unary + job.dst_off;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int yy = (int)(p / job.W), xx = (int)(p - (long long)yy * job.W);
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(yy, sh, job.h, y0, y1, ly0, ly1);
        src_index(xx, sw, job.w, x0, x1, lx0, lx1);
        const float *t00 = src + ((long long)y0 * job.w + x0) * C, *t01 = src + ((long long)y0 * job.w + x1) * C;
        const float *t10 = src + ((long long)y1 * job.w + x0) * C, *t11 = src + ((long long)y1 * job.w + x1) * C;
        float *u = dst + p;
        if (VEC4) {
            for (int c = 0; c < C; c += 4) {
                const f32x4_t a = *reinterpret_cast<const f32x4_t *>(t00 + c), b = *reinterpret_cast<const f32x4_t *>(t01 + c);
                const f32x4_t e = *reinterpret_cast<const f32x4_t *>(t10 + c), d = *reinterpret_cast<const f32x4_t *>(t11 + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) u[(long long)(c + k) * n] = -logf(bilerp4(a[k], b[k], e[k], d[k], ly0, ly1, lx0, lx1));
            }
        } else {
            for (int c = 0; c < C; ++c) u[(long long)c * n] = -logf(bilerp4(t00[c], t01[c], t10[c], t11[c], ly0, ly1, lx0, lx1));
        }
    }
}

// q: image b's [C][h*w] block at src_off; label: its H*W int32 labels at dst_off
__global__ __launch_bounds__(256) void seg_resize_argmax_kernel(const float *__restrict__ q, const SegJob *__restrict__ jobs, int C,
                                                                int32_t *__restrict__ label) {
    const SegJob job = jobs[blockIdx.y];
    const long long n = (long long)job.H * job.W, hw = (long long)job.h * job.w;
    const float sh = (float)job.h / (float)job.H, sw = (float)job.w / (float)job.W;
    const float *src = q + job.src_off;
    int32_t *dst = label + job.dst_off;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int yy = (int)(p / job.W), xx = (int)(p - (long long)yy * job.W);
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(yy, sh, job.h, y0, y1, ly0, ly1);
        src_index(xx, sw, job.w, x0, x1, lx0, lx1);
        float best = bilerp(src, job.w, y0, y1, ly0, ly1, x0, x1, lx0, lx1);
        int idx = 0;
        for (int c = 1; c < C; ++c) {
            const float v = bilerp(src + c * hw, job.w, y0, y1, ly0, ly1, x0, x1, lx0, lx1);
            if (v > best) { // strict: np.argmax keeps the first maximum
                best = v;
                idx = c;
            }
        }
        dst[p] = idx;
    }
}

// The checks both entry points share, and the job table they fill.
int seg_jobs(const char *who, int B, int C, const int64_t *src_off, const int32_t *src_hw, const int32_t *out_hw, const int64_t *dst_off,
             std::vector<SegJob> &jobs, long long *max_pix, long long *out_pix, long long *src_pix) {
    WSC_CHECK(B >= 1 && B <= 65535 && C >= 1 && C <= SEG_MAX_C, WSC_ERR_INVALID, "%s: B=%d C=%d (1 <= B <= 65535, 1 <= C <= %d)", who, B, C,
              SEG_MAX_C);
    jobs.resize(B);
    *max_pix = *out_pix = *src_pix = 0;
    for (int b = 0; b < B; ++b) {
        SegJob &j = jobs[b];
        j.h = src_hw[2 * b]; j.w = src_hw[2 * b + 1];
        j.H = out_hw[2 * b]; j.W = out_hw[2 * b + 1];
        WSC_CHECK(j.h >= 1 && j.w >= 1 && j.H >= 1 && j.W >= 1, WSC_ERR_INVALID, "%s: image %d: %dx%d -> %dx%d (every size must be >= 1)",
                  who, b, j.h, j.w, j.H, j.W);
        WSC_CHECK((long long)j.h * j.w <= INT_MAX && (long long)j.H * j.W <= INT_MAX, WSC_ERR_INVALID,
                  "%s: image %d: %dx%d -> %dx%d (an image's pixel count must fit an int32)", who, b, j.h, j.w, j.H, j.W);
        WSC_CHECK(src_off[b] >= 0 && dst_off[b] >= 0, WSC_ERR_INVALID, "%s: image %d: negative offset (%lld, %lld)", who, b,
                  (long long)src_off[b], (long long)dst_off[b]);
        j.src_off = src_off[b];
        j.dst_off = dst_off[b];
        *out_pix += (long long)j.H * j.W;
        *src_pix += (long long)j.h * j.w;
        *max_pix = std::max(*max_pix, (long long)j.H * j.W);
    }
    return WSC_OK;
}

// The job table on the device (its only section: offset 0) and the grid of both kernels: x over the largest output, y = image
int seg_stage(WscStagedTable &tab, const std::vector<SegJob> &jobs, long long max_pix, dim3 *grid) {
    tab.add(jobs);
    WSC_TRY(tab.upload());
    *grid = dim3((unsigned)std::min<long long>((max_pix + 255) / 256, 1024), (unsigned)jobs.size());
    return WSC_OK;
}

} // namespace

extern "C" {

int wsc_seg_unary_nhwc(wsc_ctx *ctx, const float *prob_dev, int B, int C, const int64_t *prob_off_host, const int32_t *src_hw_host,
                       const int32_t *out_hw_host, const int64_t *unary_off_host, float *unary_dev) {
    WSC_CHECK(ctx && prob_dev && prob_off_host && src_hw_host && out_hw_host && unary_off_host && unary_dev, WSC_ERR_INVALID,
              "wsc_seg_unary_nhwc: null argument");
    std::vector<SegJob> jobs;
    long long max_pix, out_pix, src_pix;
    WSC_TRY(seg_jobs("wsc_seg_unary_nhwc", B, C, prob_off_host, src_hw_host, out_hw_host, unary_off_host, jobs, &max_pix, &out_pix,
                     &src_pix));
    bool vec4 = C % 4 == 0 && (uintptr_t)prob_dev % 16 == 0;
    for (const SegJob &j : jobs) vec4 = vec4 && j.src_off % 4 == 0;
    WSC_HIP(hipSetDevice(ctx->device));
    WscStagedTable tab(ctx);
    dim3 grid;
    WSC_TRY(seg_stage(tab, jobs, max_pix, &grid));
    const SegJob *d = tab.at<const SegJob>(0);
    WscKernelTimer timer(ctx, WSC_K_CAM_TAIL, 4.0 * C * (double)(out_pix + src_pix));
    if (vec4) hipLaunchKernelGGL(seg_unary_nhwc_kernel<true>, grid, dim3(256), 0, ctx->stream, prob_dev, d, C, unary_dev);
    else hipLaunchKernelGGL(seg_unary_nhwc_kernel<false>, grid, dim3(256), 0, ctx->stream, prob_dev, d, C, unary_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

int wsc_seg_resize_argmax(wsc_ctx *ctx, const float *q_dev, int B, int C, const int64_t *q_off_host, const int32_t *src_hw_host,
                          const int32_t *out_hw_host, const int64_t *label_off_host, int32_t *label_dev) {
    WSC_CHECK(ctx && q_dev && q_off_host && src_hw_host && out_hw_host && label_off_host && label_dev, WSC_ERR_INVALID,
              "wsc_seg_resize_argmax: null argument");
    std::vector<SegJob> jobs;
    long long max_pix, out_pix, src_pix;
    WSC_TRY(seg_jobs("wsc_seg_resize_argmax", B, C, q_off_host, src_hw_host, out_hw_host, label_off_host, jobs, &max_pix, &out_pix,
                     &src_pix));
    WSC_HIP(hipSetDevice(ctx->device));
    WscStagedTable tab(ctx);
    dim3 grid;
    WSC_TRY(seg_stage(tab, jobs, max_pix, &grid));
    const SegJob *d = tab.at<const SegJob>(0);
    WscKernelTimer timer(ctx, WSC_K_CAM_TAIL, 4.0 * ((double)out_pix + (double)C * src_pix));
    hipLaunchKernelGGL(seg_resize_argmax_kernel, grid, dim3(256), 0, ctx->stream, q_dev, d, C, label_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

} // extern "C"
