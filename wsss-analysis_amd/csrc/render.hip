// render.hip -- wsc_render_labels: the should_saveimg debug images of every stage (03c_hsn/demo.py:183-199, :211-232, :395-418;
// 02_cues/demo.py:433-477, :604-608; 03a_sec-dsrg/model.py:596-612) for a ragged batch, in one launch:
//   pred_idx = cv2.resize(labels, out, INTER_NEAREST)            (one stage, or two: src -> mid -> out, composed per pixel)
//   pred_segmask = sum_k (pred_idx == k) * colours[k]           (one palette lookup: the masks are exclusive)
//   overlay = f((1 - R) * img + R * pred_segmask)               (a host-built table [entry][channel][image byte])
// The reference's blend is float64 numpy truncated (or, in 02_cues, rounded by imsave): the host tabulates its literal expression
// for the 256 image bytes of every palette entry and channel, and the device only looks up -- no floating-point blend here, so
// this file needs no -ffp-contract=off (the nearest index is one double product and a floor, cv2_nearest.h).
//
// render_kernel: a workgroup stages the packed palette (and the blend table, when an overlay is asked for) in LDS once and then
// walks 16-byte chunks of one image's [H][W][3] byte stream: a thread owns one aligned chunk per trip, consecutive lanes
// consecutive chunks, so every load of the image and every store is a full-width, fully coalesced 16-byte access.  A chunk
// starts `ph` bytes into pixel p0 (ph = byte position mod 3) and always touches exactly six pixels; their 24-bit colours are
// packed into five words and shifted down by ph bytes.  A packed image starts at byte 3 * pixels, which is on no 16-byte grid
// in general: the bytes in front of the first aligned chunk and behind the last one (< 16 each) go through the scalar path,
// as does the whole image when the three arrays do not share their alignment.
#include "common.h"
#include "cv2_nearest.h"

#include <limits.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int RENDER_MAX_COLOURS = 63;
constexpr int PAL_WORDS = 64;         // LDS words in front of the blend table
constexpr int CHUNKS_PER_THREAD = 16; // trips of a thread: the LDS staging (up to 48 KB) is paid once per 64 KB of output

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct RenderJob {
    long long lab_off;     // element offset of the image's label map
    long long out_off;     // byte offset of the image in colour / overlay / img
    int h, w;              // label map
    int mid_h, mid_w;      // 0, 0: one stage
    int out_h, out_w;
    double inv_y1, inv_x1; // into the label map, from mid (two stages) or from out
    double inv_y2, inv_x2; // into mid, from out (two stages only)
};

__device__ __forceinline__ int src_row(const RenderJob &job, int Y) {
    if (job.mid_h) Y = cv2_nearest_index(Y, job.inv_y2, job.mid_h);
    return cv2_nearest_index(Y, job.inv_y1, job.h);
}

// palette entry of output pixel (row with source row sy, column X): the label, or n_colours for a label outside [0, n_colours)
template <bool I32>
__device__ __forceinline__ int entry_at(const void *__restrict__ labels, const RenderJob &job, int sy, int X, int n_colours) {
    if (job.mid_w) X = cv2_nearest_index(X, job.inv_x2, job.mid_w);
    const int sx = cv2_nearest_index(X, job.inv_x1, job.w);
    const long long sp = job.lab_off + (long long)sy * job.w + sx;
    const unsigned v = I32 ? (unsigned)reinterpret_cast<const int32_t *>(labels)[sp] : (unsigned)reinterpret_cast<const uint8_t *>(labels)[sp];
    return (int)min(v, (unsigned)n_colours); // (a negative int32 is a large unsigned)
}

// six 24-bit pixels -> the five words of their byte stream
__device__ __forceinline__ void pack6(const uint32_t (&c)[6], uint32_t (&s)[5]) {
    s[0] = c[0] | (c[1] << 24);
    s[1] = (c[1] >> 8) | (c[2] << 16);
    s[2] = (c[2] >> 16) | (c[3] << 8);
    s[3] = c[4] | (c[5] << 24);
    s[4] = c[5] >> 8;
}
// the 16 bytes that start `ph` bytes into a five-word stream
__device__ __forceinline__ u32x4_t shift_down(const uint32_t (&s)[5], int ph) {
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (uint32_t)((((uint64_t)s[j + 1] << 32) | s[j]) >> (8 * ph));
    return o;
}

// pal_g: [n_colours + 1] words r | g << 8 | b << 16, the last one the 'other' colour; blend_g: [n_colours + 1][3][256] bytes
template <bool I32>
__global__ __launch_bounds__(256) void render_kernel(const void *__restrict__ labels, const RenderJob *__restrict__ jobs,
                                                     const uint32_t *__restrict__ pal_g, const uint8_t *__restrict__ blend_g,
                                                     int n_colours, int vec_ok, const uint8_t *__restrict__ img,
                                                     uint8_t *__restrict__ colour, uint8_t *__restrict__ overlay) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[]; // (the table is staged and the palette offset by whole 16 bytes)
    const RenderJob job = jobs[blockIdx.y];
    const long long nbytes = 3LL * job.out_h * job.out_w;
    uint8_t *cdst = colour + job.out_off;
    uint8_t *odst = overlay ? overlay + job.out_off : nullptr;
    const uint8_t *isrc = overlay ? img + job.out_off : nullptr;
    const long long head = vec_ok ? std::min<long long>((long long)((16u - (unsigned)((uintptr_t)cdst & 15u)) & 15u), nbytes) : nbytes;
    const long long nchunk = (nbytes - head) >> 4, tail = head + 16 * nchunk;
    const long long nscalar = head + (nbytes - tail);
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gstride = (long long)gridDim.x * blockDim.x;
    // the grid is sized by the batch's largest image: a workgroup with nothing to do in this one leaves before it stages anything
    // (the test is the same for every thread of the workgroup, so nobody is missing at the barrier below)
    const long long first = (long long)blockIdx.x * blockDim.x;
    if (first >= nchunk && first >= nscalar) return;
    uint32_t *pal = lds;
    const uint8_t *blend = reinterpret_cast<const uint8_t *>(lds + PAL_WORDS);
    for (int i = threadIdx.x; i <= n_colours; i += blockDim.x) pal[i] = pal_g[i];
    if (overlay) {
        const int n16 = (n_colours + 1) * 48; // 768 bytes per entry
        for (int i = threadIdx.x; i < n16; i += blockDim.x)
            reinterpret_cast<u32x4_t *>(lds + PAL_WORDS)[i] = reinterpret_cast<const u32x4_t *>(blend_g)[i];
    }
    __syncthreads();

    for (long long g = gtid; g < nchunk; g += gstride) {
        const long long q = head + 16 * g;
        const long long p0 = q / 3;
        const int ph = (int)(q - 3 * p0);
        int Y = (int)(p0 / job.out_w), X = (int)(p0 - (long long)Y * job.out_w);
        int sy = src_row(job, Y);
        int e[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { // (a chunk touches exactly the pixels p0 .. p0 + 5: all inside the image)
            e[k] = entry_at<I32>(labels, job, sy, X, n_colours);
            if (++X == job.out_w) {
                X = 0;
                sy = src_row(job, min(++Y, job.out_h - 1));
            }
        }
        uint32_t c[6], s[5];
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = pal[e[k]];
        pack6(c, s);
        *reinterpret_cast<u32x4_t *>(cdst + q) = shift_down(s, ph);
        if (overlay) {
            // the image's 16 bytes moved UP by ph bytes: pixel k's bytes are then bits [24 k, 24 k + 24) of the stream (the bytes
            // of the first and last pixel that lie outside the chunk read as zero; what they look up is shifted out again)
            const u32x4_t iv = *reinterpret_cast<const u32x4_t *>(isrc + q);
            uint32_t in[5];
            in[0] = (uint32_t)(((uint64_t)iv[0] << 32) >> (32 - 8 * ph));
#pragma unroll
            for (int j = 1; j < 4; ++j) in[j] = (uint32_t)((((uint64_t)iv[j] << 32) | iv[j - 1]) >> (32 - 8 * ph));
            in[4] = (uint32_t)((uint64_t)iv[3] >> (32 - 8 * ph));
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int bit = 24 * k, wd = bit >> 5, sh = bit & 31;
                uint32_t v = in[wd] >> sh;
                if (sh > 8) v |= in[wd + 1] << (32 - sh);
                const uint8_t *t = blend + e[k] * 768;
                c[k] = (uint32_t)t[v & 255u] | ((uint32_t)t[256 + ((v >> 8) & 255u)] << 8) | ((uint32_t)t[512 + ((v >> 16) & 255u)] << 16);
            }
            pack6(c, s);
            *reinterpret_cast<u32x4_t *>(odst + q) = shift_down(s, ph);
        }
    }

    // the bytes in front of the first chunk and behind the last one, one byte per thread and trip
    for (long long i = gtid; i < nscalar; i += gstride) {
        const long long q = i < head ? i : tail + (i - head);
        const long long p = q / 3;
        const int ch = (int)(q - 3 * p);
        const int Y = (int)(p / job.out_w), X = (int)(p - (long long)Y * job.out_w);
        const int e = entry_at<I32>(labels, job, src_row(job, Y), X, n_colours);
        cdst[q] = (uint8_t)(pal[e] >> (8 * ch));
        if (overlay) odst[q] = blend[(e * 3 + ch) * 256 + isrc[q]];
    }
}

} // namespace

extern "C" {

int wsc_render_labels(wsc_ctx *ctx, const void *labels_dev, int label_type, int B, const int32_t *src_hw_host,
                      const int32_t *mid_hw_host, const int32_t *out_hw_host, const int64_t *labels_off_host,
                      const int64_t *out_off_host, const uint8_t *palette_host, int n_colours, const uint8_t *other_rgb_host,
                      const uint8_t *img_dev, const uint8_t *blend_host, uint8_t *colour_dev, uint8_t *overlay_dev) {
    WSC_CHECK(ctx != nullptr, WSC_ERR_INVALID, "wsc_render_labels: null context");
    WSC_CHECK(labels_dev != nullptr, WSC_ERR_INVALID, "wsc_render_labels: labels_dev is null");
    WSC_CHECK(src_hw_host != nullptr, WSC_ERR_INVALID, "wsc_render_labels: src_hw_host is null");
    WSC_CHECK(out_hw_host != nullptr, WSC_ERR_INVALID, "wsc_render_labels: out_hw_host is null");
    WSC_CHECK(labels_off_host != nullptr, WSC_ERR_INVALID, "wsc_render_labels: labels_off_host is null");
    WSC_CHECK(out_off_host != nullptr, WSC_ERR_INVALID, "wsc_render_labels: out_off_host is null");
    WSC_CHECK(palette_host != nullptr, WSC_ERR_INVALID, "wsc_render_labels: palette_host is null");
    WSC_CHECK(other_rgb_host != nullptr, WSC_ERR_INVALID, "wsc_render_labels: other_rgb_host is null");
    WSC_CHECK(colour_dev != nullptr, WSC_ERR_INVALID, "wsc_render_labels: colour_dev is null");
    WSC_CHECK(!overlay_dev || img_dev, WSC_ERR_INVALID, "wsc_render_labels: img_dev is null (an overlay needs the image)");
    WSC_CHECK(!overlay_dev || blend_host, WSC_ERR_INVALID, "wsc_render_labels: blend_host is null (an overlay needs the blend table)");
    WSC_CHECK(label_type == WSC_RENDER_LABELS_U8 || label_type == WSC_RENDER_LABELS_I32, WSC_ERR_INVALID,
              "wsc_render_labels: label_type=%d (0 uint8, 1 int32)", label_type);
    WSC_CHECK(B >= 1 && B <= 65535, WSC_ERR_INVALID, "wsc_render_labels: B=%d (1 <= B <= 65535)", B);
    WSC_CHECK(n_colours >= 1 && n_colours <= RENDER_MAX_COLOURS, WSC_ERR_INVALID, "wsc_render_labels: n_colours=%d (1 <= n_colours <= %d)",
              n_colours, RENDER_MAX_COLOURS);
    std::vector<RenderJob> jobs(B);
    long long max_bytes = 0;
    double work = 0;
    for (int b = 0; b < B; ++b) {
        RenderJob &j = jobs[b];
        j.h = src_hw_host[2 * b]; j.w = src_hw_host[2 * b + 1];
        j.out_h = out_hw_host[2 * b]; j.out_w = out_hw_host[2 * b + 1];
        j.mid_h = mid_hw_host ? mid_hw_host[2 * b] : 0;
        j.mid_w = mid_hw_host ? mid_hw_host[2 * b + 1] : 0;
        WSC_CHECK(j.h >= 1 && j.w >= 1 && (long long)j.h * j.w <= INT_MAX, WSC_ERR_INVALID,
                  "wsc_render_labels: image %d: src_hw %d x %d (both >= 1, h * w within int32)", b, j.h, j.w);
        WSC_CHECK(j.out_h >= 1 && j.out_w >= 1 && (long long)j.out_h * j.out_w <= INT_MAX, WSC_ERR_INVALID,
                  "wsc_render_labels: image %d: out_hw %d x %d (both >= 1, h * w within int32)", b, j.out_h, j.out_w);
        WSC_CHECK((j.mid_h == 0 && j.mid_w == 0) || (j.mid_h >= 1 && j.mid_w >= 1 && (long long)j.mid_h * j.mid_w <= INT_MAX), WSC_ERR_INVALID,
                  "wsc_render_labels: image %d: mid_hw %d x %d (0 x 0 for one stage, else both >= 1 and h * w within int32)", b, j.mid_h,
                  j.mid_w);
        WSC_CHECK(labels_off_host[b] >= 0, WSC_ERR_INVALID, "wsc_render_labels: image %d: labels_off %lld is negative", b,
                  (long long)labels_off_host[b]);
        WSC_CHECK(out_off_host[b] >= 0, WSC_ERR_INVALID, "wsc_render_labels: image %d: out_off %lld is negative", b,
                  (long long)out_off_host[b]);
        j.lab_off = labels_off_host[b];
        j.out_off = out_off_host[b];
        if (j.mid_h) {
            j.inv_y1 = cv2_nearest_inv(j.h, j.mid_h); j.inv_x1 = cv2_nearest_inv(j.w, j.mid_w);
            j.inv_y2 = cv2_nearest_inv(j.mid_h, j.out_h); j.inv_x2 = cv2_nearest_inv(j.mid_w, j.out_w);
        } else {
            j.inv_y1 = cv2_nearest_inv(j.h, j.out_h); j.inv_x1 = cv2_nearest_inv(j.w, j.out_w);
            j.inv_y2 = j.inv_x2 = 1.0;
        }
        const long long nbytes = 3LL * j.out_h * j.out_w;
        max_bytes = std::max(max_bytes, nbytes);
        work += (double)nbytes * (overlay_dev ? 3 : 1) + (double)j.h * j.w * (label_type == WSC_RENDER_LABELS_I32 ? 4 : 1);
    }
    std::vector<uint32_t> pal(n_colours + 1);
    for (int k = 0; k <= n_colours; ++k) {
        const uint8_t *c = k < n_colours ? palette_host + 3 * k : other_rgb_host;
        pal[k] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
    }
    WSC_HIP(hipSetDevice(ctx->device));
    WscStagedTable tab(ctx);
    const size_t jo = tab.add(jobs), po = tab.add(pal);
    const size_t bo = tab.add(overlay_dev ? blend_host : nullptr, overlay_dev ? (size_t)(n_colours + 1) * 768 : 0);
    WSC_TRY(tab.upload());
    // 16-byte accesses need the three arrays on one 16-byte grid (they share the byte offsets)
    const uintptr_t cp = (uintptr_t)colour_dev, op = (uintptr_t)overlay_dev, ip = (uintptr_t)img_dev;
    const int vec_ok = !overlay_dev || (((cp ^ op) & 15u) == 0 && ((cp ^ ip) & 15u) == 0);
    const long long per_block = 256LL * 16 * CHUNKS_PER_THREAD;
    const dim3 grid((unsigned)std::min<long long>(std::max<long long>((max_bytes + per_block - 1) / per_block, 1), 4096), (unsigned)B);
    // <= 256 + 64 * 768 = 49408 bytes: inside the 64 KB a workgroup may ask for without hipFuncAttributeMaxDynamicSharedMemorySize
    // (wsc_set_max_dynamic_lds is for the kernels that go beyond it)
    const size_t lds_bytes = PAL_WORDS * sizeof(uint32_t) + (overlay_dev ? (size_t)(n_colours + 1) * 768 : 0);
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, work);
    if (label_type == WSC_RENDER_LABELS_I32)
        hipLaunchKernelGGL(render_kernel<true>, grid, dim3(256), lds_bytes, ctx->stream, labels_dev, tab.at<const RenderJob>(jo),
                           tab.at<const uint32_t>(po), tab.at<const uint8_t>(bo), n_colours, vec_ok, img_dev, colour_dev, overlay_dev);
    else
        hipLaunchKernelGGL(render_kernel<false>, grid, dim3(256), lds_bytes, ctx->stream, labels_dev, tab.at<const RenderJob>(jo),
                           tab.at<const uint32_t>(po), tab.at<const uint8_t>(bo), n_colours, vec_ok, img_dev, colour_dev, overlay_dev);
    WSC_HIP(hipGetLastError());
    tab.release(); // stream-ordered reuse
    return WSC_OK;
}

} // extern "C"
