// dsrg.hip -- DSRG seeded region growing on the device (03a_sec-dsrg/DSRG.py:7-62 single_generate_seed_step, batch driver
// :356-371).  Per image: e = prob * tag; a = argmax_c e (first maximum); the pixel's candidate class by the mask arithmetic
// of :28-39; per tagged class c the 8-connected components of mat_c = {candidate == c}; a component that holds a pixel with
// cue[p][c] == 1 is grown: cue[p][c] = 1 on all of it except the pixels that are already seeded for exactly one other class
// (sum_k cue[p][k] == 1 and cue[p][c] != 1).  Those still take part in connectivity -- they can bridge two halves.
//
// ASSUMPTION: lib/CC_labeling_8.py, the reference's labeller, is not in the reference tree.  By its name and upstream DSRG
// connectivity is 8-neighbour, label 0 means "not in mat_c", and such pixels are never filled.
//
//   dsrg_classify_kernel  one thread per pixel: the candidate class, whether the pixel is a seed of it, whether it is blocked
//                         -- everything a pixel contributes, for the ONE class it can belong to -- as one byte of a scratch
//                         plane [B][H*W]; copies cues to out when the two differ
//   dsrg_grow_kernel      one workgroup per (class, image): label plane in LDS, seeded with the pixel index; "minimum over the
//                         8 neighbours inside mat_c, lower the pixel's root to it, compress the chains" until a workgroup-wide
//                         vote says that nothing changed; one LDS flag per root marks the components with a seed
// cue values are 0/1 as the reference's are (the sum over classes is then exact in any order).
#include "common.h"

namespace {

constexpr int DSRG_MAX_C = 32;         // classes (wsc_crf_inference's bound on M)
constexpr int DSRG_MAX_PIXELS = 8192;  // H * W: 4-byte label + 1-byte root flag per pixel = 40 KiB of the 64 KiB a launch gets
                                       // without raising the dynamic-LDS attribute
constexpr int DSRG_GROW_THREADS = 512;
constexpr int DSRG_NOT_MEMBER = 0x7fffffff; // label of a pixel outside mat_c: never the minimum
// scratch byte of a pixel
constexpr unsigned DSRG_CLASS_MASK = 0x3f, DSRG_NO_CLASS = 0x3f; // (classes are < 32)
constexpr unsigned DSRG_SEED = 0x40;    // cue[p][class] == 1
constexpr unsigned DSRG_BLOCKED = 0x80; // not a seed, and seeded for exactly one other class

// cues and out may be the same buffer (then `copy` is 0 and out is not touched here): no __restrict__ on the two
__global__ void dsrg_classify_kernel(const float *__restrict__ tags, const float *cues, const float *__restrict__ probs, int HW,
                                     int C, float th_f, float th_b, int copy, uint8_t *__restrict__ code, float *out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const float *tag = tags + (size_t)b * C;
    const size_t at = ((size_t)b * HW + p) * C;
    const float *pr = probs + at, *cu = cues + at;
    float best = pr[0] * tag[0];
    const bool bg_over = best > th_b; // (existing_prob[:, :, 0:1] > th_b), :35
    bool fg_over = false;             // any (existing_prob[:, :, 1:] > th_f), :33
    int a = 0;
    for (int k = 1; k < C; ++k) {
        const float e = pr[k] * tag[k];
        fg_over |= e > th_f;
        if (e > best) { // strict: np.argmax keeps the first maximum
            best = e;
            a = k;
        }
    }
    // label_map = (fg_th * is_fg + bg_th * (1 - is_fg)) * (argmax + 1), :38-39
    const bool has = a >= 1 ? fg_over : bg_over;
    float sum = 0.f;
    for (int k = 0; k < C; ++k) {
        const float v = cu[k];
        sum += v;
        if (copy) out[at + k] = v;
    }
    unsigned c = DSRG_NO_CLASS;
    if (has) {
        c = (unsigned)a;
        if (cu[a] == 1.f) c |= DSRG_SEED; // :55
        else if (sum == 1.f) c |= DSRG_BLOCKED; // :57
    }
    code[(size_t)b * HW + p] = (uint8_t)c;
}

// grid (C, B).  LDS: int label[HW], then uint8 hot[HW] (hot[r]: the component whose root is pixel r holds a seed).
__global__ __launch_bounds__(DSRG_GROW_THREADS) void dsrg_grow_kernel(const float *__restrict__ tags,
                                                                      const uint8_t *__restrict__ code, int H, int W, int C,
                                                                      float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char dsrg_lds[];
    const int c = blockIdx.x, b = blockIdx.y, HW = H * W;
    if (!(tags[(size_t)b * C + c] > 0.5f)) return; // cls_index = np.where(tag > 0.5), :47
    int *label = (int *)dsrg_lds;
    uint8_t *hot = (uint8_t *)(label + HW);
    const uint8_t *cd = code + (size_t)b * HW;

    int seeds = 0;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        const unsigned v = cd[p];
        const bool member = (v & DSRG_CLASS_MASK) == (unsigned)c;
        label[p] = member ? p : DSRG_NOT_MEMBER;
        hot[p] = 0;
        seeds |= member && (v & DSRG_SEED);
    }
    if (!__syncthreads_or(seeds)) return; // no seed of this class: nothing grows

    // Labels are pixel indices of the pixel's own component and only ever decrease; label[r] == r makes r a root.  A scan
    // that finds a smaller label next to p lowers p's ROOT to it (atomicMin: several pixels may lower one root), so the news
    // reaches the whole tree in the compress that follows instead of walking it pixel by pixel -- a serpentine takes a handful
    // of rounds.  The loop ends on the first scan that changes nothing: then no pixel has a neighbour with a smaller label,
    // so labels are constant on every component, and after the last compress each is its component's root.
    for (;;) {
        int changed = 0;
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int l = label[p];
            if (l == DSRG_NOT_MEMBER) continue;
            const int y = p / W, x = p - y * W; // neighbours by (row, column): a row end has no neighbour in the next row
            int m = l;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= W) continue;
                    m = min(m, label[yy * W + xx]);
                }
            }
            if (m < l) {
                atomicMin(&label[l], m);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            int r = label[p];
            if (r == DSRG_NOT_MEMBER) continue;
            for (int n = label[r]; n != r; n = label[r]) r = n; // (chains only get shorter under the other threads' writes)
            label[p] = r;
        }
        __syncthreads();
    }

    for (int p = threadIdx.x; p < HW; p += blockDim.x)
        if (label[p] != DSRG_NOT_MEMBER && (cd[p] & DSRG_SEED)) hot[label[p]] = 1;
    __syncthreads();
    float *o = out + (size_t)b * HW * C + c;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        const int l = label[p];
        // seeds are 1 already; blocked pixels stay as they are (:57-58)
        if (l != DSRG_NOT_MEMBER && hot[l] && !(cd[p] & (DSRG_SEED | DSRG_BLOCKED))) o[(size_t)p * C] = 1.f;
    }
}

} // namespace

extern "C" {

int wsc_dsrg_seed_grow(wsc_ctx *ctx, const float *tags_dev, const float *cues_dev, const float *probs_dev, int B, int H, int W, int C,
                       float th_f, float th_b, float *out_dev) {
    WSC_CHECK(ctx && tags_dev && cues_dev && probs_dev && out_dev, WSC_ERR_INVALID, "wsc_dsrg_seed_grow: null argument");
    WSC_CHECK(B > 0 && H > 0 && W > 0 && C >= 1 && C <= DSRG_MAX_C, WSC_ERR_INVALID,
              "wsc_dsrg_seed_grow: B=%d H=%d W=%d C=%d (sizes must be positive, C <= %d)", B, H, W, C, DSRG_MAX_C);
    WSC_CHECK((long long)H * W <= DSRG_MAX_PIXELS && B <= 65535, WSC_ERR_INVALID,
              "wsc_dsrg_seed_grow: H=%d x W=%d = %lld pixels, B=%d (an image's label plane lives in LDS: at most %d pixels; B <= 65535)",
              H, W, (long long)H * W, B, DSRG_MAX_PIXELS);
    WSC_HIP(hipSetDevice(ctx->device));
    const int HW = H * W;
    uint8_t *code = nullptr;
    WSC_TRY(wsc_ctx_cached_alloc(ctx, (size_t)B * HW, (void **)&code));
    WscCachedGuard code_guard(ctx, code);
    const int copy = out_dev != cues_dev ? 1 : 0;
    WscKernelTimer timer(ctx, WSC_K_POOL_MISC, (double)B * HW * (4.0 * C * (2 + copy) + 2));
    // In place (out_dev == cues_dev) is safe.  The grow kernel reads the scratch plane only, which the classify kernel has
    // finished before it starts (one stream), and it is the reference's own order of events: the candidate sets of different
    // classes are disjoint, class c writes cue[p][c] on its own pixels only and reads cue[p][:] on its own pixels only, so the
    // reference's in-place loop over classes (:48-61) sees, for every pixel it tests, the cues as they were before the call.
    hipLaunchKernelGGL(dsrg_classify_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, ctx->stream, tags_dev, cues_dev, probs_dev, HW,
                       C, th_f, th_b, copy, code, out_dev);
    WSC_HIP(hipGetLastError());
    const size_t lds = (size_t)HW * (sizeof(int) + 1);
    hipLaunchKernelGGL(dsrg_grow_kernel, dim3(C, B), dim3(DSRG_GROW_THREADS), lds, ctx->stream, tags_dev, (const uint8_t *)code, H, W,
                       C, out_dev);
    WSC_HIP(hipGetLastError());
    code_guard.free_now();
    return WSC_OK;
}

} // extern "C"
