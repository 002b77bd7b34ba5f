// common.h -- shared declarations of libwsscam (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stdint.h>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/wsscam.h"

typedef uint16_t bf16_t; // raw bfloat16 bits

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// ---- bf16 helpers (host + device), round-to-nearest-even --------------------
__host__ __device__ inline bf16_t f32_to_bf16(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    uint32_t u = v.u;
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40); // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
__host__ __device__ inline float bf16_to_f32(bf16_t h) {
    union { float f; uint32_t u; } v;
    v.u = ((uint32_t)h) << 16;
    return v.f;
}

// ---- IEEE half helpers: round-to-nearest-even, SATURATING at +-65504 (no infinities) -------
// NaN: the host form keeps it (0x7e00), the device form stores -65504 (fmaxf / fminf return the other operand) -- at the ceiling,
// so every site that tests half2_at_ceiling or |v| < 65504 flags it.  They need not agree: no NaN passes the host form, make_conv
// rejects a non-finite weight, scale or shift of an IEEE-half model before it packs.
__host__ __device__ inline uint16_t f32_to_f16(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)fminf(fmaxf(f, -65504.f), 65504.f);
    return __builtin_bit_cast(uint16_t, h);
#else
    union { float f; uint32_t u; } v, magic;
    v.f = f;
    const uint32_t sign = v.u & 0x80000000u;
    v.u ^= sign;
    uint16_t o;
    if (v.u >= ((127u + 16u) << 23)) {
        o = v.u > (255u << 23) ? 0x7e00 : 0x7bff; // NaN stays NaN, overflow saturates
    } else if (v.u < (113u << 23)) { // subnormal half or zero
        magic.u = ((127u - 15u) + (23u - 10u) + 1u) << 23;
        v.f += magic.f;
        o = (uint16_t)(v.u - magic.u);
    } else {
        const uint32_t mant_odd = (v.u >> 13) & 1u;
        v.u += ((15u - 127u) << 23) + 0xfffu;
        v.u += mant_odd;
        o = (uint16_t)(v.u >> 13);
        if (o >= 0x7c00) o = 0x7bff;
    }
    return (uint16_t)(o | (sign >> 16));
#endif
}
__host__ __device__ inline float f16_to_f32(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, h);
#else
    union { float f; uint32_t u; } o, magic;
    magic.u = 113u << 23;
    const uint32_t shifted_exp = 0x7c00u << 13;
    o.u = ((uint32_t)h & 0x7fffu) << 13;
    const uint32_t exp = shifted_exp & o.u;
    o.u += (127u - 15u) << 23;
    if (exp == shifted_exp) o.u += (128u - 16u) << 23;
    else if (exp == 0) { o.u += 1u << 23; o.f -= magic.f; }
    o.u |= ((uint32_t)h & 0x8000u) << 16;
    return o.f;
#endif
}
// 16-bit storage format of activations / weights: 0 = bfloat16, 1 = IEEE half
__host__ __device__ inline uint16_t f32_to_h16(float f, int fmt) { return fmt ? f32_to_f16(f) : f32_to_bf16(f); }
__host__ __device__ inline float h16_to_f32(uint16_t h, int fmt) { return fmt ? f16_to_f32(h) : bf16_to_f32(h); }

// ReLU and maximum that carry a NaN like torch / TensorFlow do (fmaxf returns the other operand): what the bf16, bf16x3 and fp32
// paths propagate, and what keeps a NaN in front of the saturating half conversion where it is flagged
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float max_keep_nan(float a, float b) { return (b > a || b != b) ? b : a; }

// ---- error plumbing -----------------------------------------------------------
void wsc_set_error(const char *fmt, ...);
#define WSC_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            wsc_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr,                   \
                          hipGetErrorString(_e));                                              \
            return WSC_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)
#define WSC_CHECK(cond, code, ...)                                                             \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            wsc_set_error(__VA_ARGS__);                                                        \
            return (code);                                                                     \
        }                                                                                      \
    } while (0)
#define WSC_TRY(expr)                                                                          \
    do {                                                                                       \
        int _s = (expr);                                                                       \
        if (_s != WSC_OK) return _s;                                                           \
    } while (0)

// ---- per-kernel-class timing (wsc_profile_begin / _end) --------------------------------------------
enum WscKernelClass {
    WSC_K_CONV256 = 0,   // conv_igemm_kernel, 256x256 tile
    WSC_K_CONV128,       // conv_igemm_kernel, 128x128 tile, LDS-DMA staging (and conv_f32_kernel's, like the two classes below)
    WSC_K_CONV64,        // conv_igemm_kernel, 128x64 tile
    WSC_K_CONV_SMALLCIN, // conv_igemm_kernel, stem / first layer (register staging); stem_pool_kernel (f16x3 ResNet stem + max-pool)
    WSC_K_POOL_MISC,     // maxpool, layout changes, flip-add, classifier branch
    WSC_K_CAM_TAIL,      // cam_tail_kernel (both passes) + unary_from_maps
    WSC_K_CRF_BUILD,     // every kernel of wsc_crf_create
    WSC_K_GAUSS_MSG,     // gauss_msg_kernel: Gaussian lattice combine + three blur passes + slice into E, per pixel tile, in LDS
    WSC_K_BLUR,          // combine4_kernel + blur4_kernel (bilateral) + blur3_tile_kernel (Gaussian, when its message is not formed on chip)
    WSC_K_SLICE_UPDATE,  // update_splat_kernel: slice + mean-field update + splat of the result
    WSC_K_CRF_MISC,      // init_q / finish
    WSC_K_WGRAD,         // wgrad_kernel + wgrad_reduce_kernel (seg_grad.hip); work = algorithmic FLOPs
    WSC_K_GRAD_MISC,     // ReLU mask + bias gradient, pool gradients, channel copies of the backward pass
    WSC_K_UPSAMPLE_GRAD, // relu_up_grad_kernel (irn_grad.hip)
    WSC_K_GN_GRAD,       // gn_grad_partial / columns / finish / apply kernels (irn_grad.hip)
    WSC_K_COUNT
};
struct WscProfRecord {
    int cls;
    double work; // algorithmic FLOPs (conv classes) or bytes (everything else) of this launch
    hipEvent_t e0, e1;
};

// ---- context --------------------------------------------------------------------
struct WscGaussCache; // crf.hip
void wsc_gauss_cache_destroy(WscGaussCache *cache);
struct wsc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 0;
    std::string arch;
    // grow-only workspace arena (activations, CRF scratch); never freed before destroy
    void *ws = nullptr;
    size_t ws_bytes = 0;
    // small pinned staging buffers for descriptor uploads: a ring of slots, so that an upload waits for an earlier one only
    // when the ring has gone round (a copy is ordered behind everything enqueued on the stream before it: with one slot the
    // host blocked on the previous call's whole device work)
    static constexpr int PIN_SLOTS = 8;
    struct PinSlot {
        void *p = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr; // completion of the last copy out of this slot
        bool busy = false;
    };
    PinSlot pin_ring[PIN_SLOTS];
    int pin_next = 0;
    // path selectors (wsc_ctx_set_option): every one picks between two paths that both exist for some inputs and give the
    // same bits -- the tests hold them to that -- with ONE exception: WSC_OPT_CAM_HEAD_STREAM.  cam_head_kernel sums K in four
    // per-wave quarters, a different fp32 summation order from the tiled kernel: equal to fp32 round-off (test bound 2e-6
    // relative), not bit-identical.  Defaults: wsc_option in include/wsscam.h.
    int opt[WSC_OPT_COUNT] = {1, 1, 1, 0, 0, -1, 1, 1, 1, 1};
    void *zero_page = nullptr; // 256 bytes of zeros in HBM (source of padded conv taps)
    // range guard of the IEEE-half conv modes: one word of mapped, page-locked host memory that a conv epilogue stores to
    // (plain store of a non-zero value, no atomic needed: every writer writes "raised") when an activation saturates at the
    // half ceiling; read by the host after a stream synchronisation (wsc_sync, wsc_memcpy_d2h, wsc_ctx_range_status)
    unsigned *range_host = nullptr, *range_dev = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t join_ev = nullptr; // wsc_ctx_wait
    hipEvent_t marks[8] = {};     // wsc_ctx_mark / wsc_ctx_wait_mark (created on first use)
    bool mark_set[8] = {};
    // side stream for work that is independent inside one call (crf.hip: the bilateral lattice's combine + blur passes run
    // beside the Gaussian lattice's fused blur); forked from / joined into `stream` with the two events
    hipStream_t aux_stream = nullptr;
    hipEvent_t fork_ev = nullptr, aux_done_ev = nullptr;
    bool profiling = false;
    std::vector<WscProfRecord> prof;
    std::vector<hipEvent_t> prof_pool;
    // stream-ordered caching allocator: blocks released by wsc_ctx_cached_free are reused by later
    // requests of the same ctx (all work of a ctx is on one stream, so reuse is ordered after the
    // previous user) instead of going through hipFree/hipMalloc (both synchronise the device).
    std::multimap<size_t, void *> free_blocks;
    std::unordered_map<void *, size_t> live_blocks;
    // crf.hip's per-image-size Gaussian lattices (created by the first wsc_crf_create); their device arrays are cached-alloc
    // blocks, handed back when the cache is destroyed and freed with everything else at destroy
    WscGaussCache *gauss_cache = nullptr;
    // wsc_ctx_scratch_fill: -1 = off, else the byte that the arena (on the call and at every request), every cached block
    // handed out and the grad objects' own workspaces (net.hip, repack.hip) are set to.  Not a path selector: a test hook that
    // makes a read of scratch nobody wrote show up in values
    int scratch_fill = -1;
};
int wsc_ctx_workspace(wsc_ctx *ctx, size_t bytes, void **out);
// WSC_ERR_RANGE (with the error text) when the ctx's range flag is raised; the stream must have been synchronised
int wsc_ctx_range_check(wsc_ctx *ctx);
// One packed pair of IEEE halves as the saturation test of an epilogue: bit 15 / 31 of the result is set iff the low / high
// half's magnitude is >= 0x7bff (65504: the value the saturating conversion stores for anything beyond, +-inf included; a half
// NaN or inf pattern, which no conversion of this library stores, tests true as well).  An fp32 NaN reaches this test only where
// the conversion in front of it keeps it out of a ReLU: f32_to_f16's device form stores -65504 for it (flagged), the median
// of the FAST epilogues stores its lower bound -- 0 under ReLU, NOT flagged.  The IEEE-half modes therefore keep NaN / inf out at
// the doors (the packs above, make_conv, the device repack); finite halves and fp32 accumulators cannot form one in flight.
__device__ __forceinline__ unsigned half2_at_ceiling(unsigned hw) { return (hw & 0x7fff7fffu) + 0x04010401u; }
// Brackets the launches enqueued during its lifetime with a pair of HIP events on the ctx stream
// when profiling is on (no-op otherwise).
struct WscKernelTimer {
    wsc_ctx *ctx;
    int idx = -1;
    WscKernelTimer(wsc_ctx *c, int cls, double work);
    ~WscKernelTimer();
};
int wsc_ctx_cached_alloc(wsc_ctx *ctx, size_t bytes, void **out);
void wsc_ctx_cached_free(wsc_ctx *ctx, void *p);
// Scope guard of a cached block: an early `return` of WSC_TRY / WSC_HIP / WSC_CHECK gives the block back too
// (free_now() at the usual place keeps the stream-ordered reuse exactly where it was).
struct WscCachedGuard {
    wsc_ctx *ctx;
    void *p;
    WscCachedGuard(wsc_ctx *c, void *q) : ctx(c), p(q) {}
    WscCachedGuard(const WscCachedGuard &) = delete;
    WscCachedGuard &operator=(const WscCachedGuard &) = delete;
    void free_now() {
        if (p) wsc_ctx_cached_free(ctx, p);
        p = nullptr;
    }
    ~WscCachedGuard() { free_now(); }
};
// copies `bytes` of host data to dst_dev through the ctx's pinned staging buffer, asynchronously
int wsc_ctx_upload_small(wsc_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
// A small host-built table on the device for ONE call (the per-image jobs of a ragged batch, their keys, zeroed counters or
// maxima): add() the sections, upload() them as one cached block through one pinned-ring copy, hand at<T>(offset) to the
// launches, release() after the last launch that reads the table (stream-ordered reuse, as WscCachedGuard::free_now()).  An
// early `return` of WSC_TRY / WSC_HIP / WSC_CHECK gives the block back too.  Only read_back() synchronises.
class WscStagedTable {
  public:
    explicit WscStagedTable(wsc_ctx *c) : ctx(c) {}
    WscStagedTable(const WscStagedTable &) = delete;
    WscStagedTable &operator=(const WscStagedTable &) = delete;
    ~WscStagedTable() { release(); }
    // appends a 16-byte aligned section, returns its byte offset; src == nullptr: zeros; an empty section is legal and free
    size_t add(const void *src, size_t bytes);
    template <class T> size_t add(const std::vector<T> &v) { return add(v.data(), v.size() * sizeof(T)); }
    int upload();
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(dev + off); }
    // device -> host copy of part of the table, then a stream synchronisation (the out-of-range counters)
    int read_back(size_t off, void *dst, size_t bytes);
    void release() { wsc_ctx_cached_free(ctx, dev); dev = nullptr; }
  private:
    wsc_ctx *ctx;
    std::vector<char> host;
    char *dev = nullptr;
};
// v[k] summed over the workgroup (a multiple of 64 threads), in every thread, in ONE order: xor butterfly inside a wave, then the
// waves in wave order (seg_loss.hip, irn_loss.hip).  Every thread of the workgroup calls it; scratch: (waves) * NV doubles of LDS.
template <int NV> __device__ __forceinline__ void block_sum(double (&v)[NV], double *scratch) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64); // a + b == b + a: the lanes agree to the bit
    const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    __syncthreads(); // (an earlier call's readers are done with scratch)
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NV; ++k) scratch[wave * NV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = 0.0;
        for (int w = 0; w < n_waves; ++w) s += scratch[w * NV + k];
        v[k] = s;
    }
}
// "The last block to arrive adds the partials": every block of a group of `n` stores its partial sums with plain stores, the block
// that finds itself last reads all n of them and finishes, in block order -- a fixed order without a second launch.  `ticket`
// counts the arrivals; the launcher zeroes it in front of every launch.  The memory-ordering argument, stated once:
//   ticket_publish   by EVERY thread that has just stored a partial.  The agent-scope release writes the thread's stores back to
//                    where every CU of the device reads them; the wait holds the wave until they have left (the compiler may
//                    drop the fence's own wait, so it is spelled, behind the fence).  Where the storing threads are not the one
//                    that takes the ticket, a __syncthreads() stands between the two calls.
//   ticket_is_last   by ONE thread of the block, behind the above.  The increment is relaxed: it orders nothing, it only
//                    counts, and it is an atomic at agent scope, so the n blocks see n different values.  Whoever draws n - 1
//                    knows that every other block's publish is complete, because each incremented behind its own.  Its acquire
//                    drops what this CU's cache may hold of the partials, and the wait holds the wave until that is done: the
//                    block's loads behind the caller's next __syncthreads() read what the other blocks wrote.  The other blocks
//                    read nothing and pay for no acquire.
// The caller hands the result to the block through LDS and that __syncthreads().
__device__ __forceinline__ void ticket_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ bool ticket_is_last(unsigned *ticket, unsigned n) {
    const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n - 1;
    if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return last;
}

// float -> uint32 whose unsigned order is the float order (-0 counts as +0: equal values must tie), and back: the sort keys of
// seg_loss.hip and cls_head.hip
__device__ __forceinline__ uint32_t float_order_bits(float v) {
    const uint32_t u = __float_as_uint(v + 0.f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float float_from_order_bits(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// Raises the dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) of kernel `fn` to `bytes`, once per (function,
// ctx device), under a lock: the lane threads of the drivers reach the launch sites at the same time.  WSC_ERR_HIP with the
// error text when the runtime refuses; a failure is not recorded, so the next call tries again.
int wsc_set_max_dynamic_lds(wsc_ctx *ctx, const void *fn, int bytes);

// ---- conv (implicit GEMM) -----------------------------------------------------------
// A wsc_precision as the kernels see it: the 16-bit format of both planes, and what the second ("lo") plane does
// (WSC_PREC_F32: one plane of fp32 -- no 16-bit format at all, conv_f32.hip and the _f32 kernels of misc / irn_kernels.hip)
constexpr int CONV_FMT_F32 = 2;
inline int conv_fmt(wsc_precision prec) { // 0 bf16, 1 IEEE half, CONV_FMT_F32
    if (prec == WSC_PREC_F32) return CONV_FMT_F32;
    return (prec == WSC_PREC_F16 || prec == WSC_PREC_F16X3) ? 1 : 0;
}
// bytes of one activation / packed-weight element of a plane: THE helper every size of such a buffer goes through
inline size_t conv_elem_bytes(wsc_precision prec) { return prec == WSC_PREC_F32 ? sizeof(float) : sizeof(bf16_t); }
// 0: one plane; 1: bf16x3 (three K segments); 2: f16x3 (hi + lo staged once per K-step where the layer is LDS-DMA staged)
inline int conv_split(wsc_precision prec) { return prec == WSC_PREC_BF16X3 ? 1 : (prec == WSC_PREC_F16X3 ? 2 : 0); }

// How a layer's input reaches the kernel
enum ConvForm {
    CONV_FORM_GENERIC = 0, // [N][H][W][Cin], Cin % 64 == 0: LDS-DMA staging, a K-step = one tap of one channel chunk
    CONV_FORM_SMALL2,      // Cin <= 4 as NHWC4, register staging: a kernel row = 2 slots of (2 pixels x 4 channels) (3 x 3 first conv)
    CONV_FORM_SMALL4,      // the same with 4 slots per kernel row (7 x 7 stem)
    CONV_FORM_STEM_ROWS    // f16x3 stem on a zero-PADDED NHWC4 input (H, W = the padded size, pad = 0): the 8-pixel x 4-channel window
                           // of kernel row r of an output pixel is 32 contiguous elements of either plane, 16-byte aligned (even
                           // stride: the window starts at an even pixel), so a K-step = one kernel row = 32 hi + 32 lo values and the
                           // layer is an LDS-DMA layer of kh K-steps with no bounds tests (the padding is in the buffer)
};
inline bool conv_form_dma(ConvForm f) { return f == CONV_FORM_GENERIC || f == CONV_FORM_STEM_ROWS; }

// K layout of a layer's packed weights [CoutPad][Kw] (16-bit; fp32 in WSC_PREC_F32) and of the kernel's K loop: THE description
// both the packing (net.hip make_conv) and the launches (conv_igemm.hip, conv_f32.hip) read.  A K-step is 128 bytes per output
// channel: `kstep` = 64 16-bit or 32 fp32 weight elements.
//   generic: K order (cin / ck, kh, kw, cin % ck) -- the kh * kw taps of one channel chunk are consecutive K-steps, so the
//            activation lines a block gathers are re-touched within a few K-steps (L2 hits) instead of Cin / ck steps later
//   small-Cin forms: kernel row r owns 4 (SMALL2) or 8 (SMALL4) pixels x 4 channels, i.e. 2 / 4 16-byte slots of 16-bit values
//            or 4 / 8 of fp32 values, 8 slots per K-step
//   stem rows: K-step r = kernel row r, 8 pixels x 4 channels (pixel 7 and channel 3: zero weights)
// Two planes: interleaved (f16x3, LDS-DMA layers) = every K-step holds [32 hi | 32 lo] of a 32-channel chunk and the K loop
// runs once; else [hi K | lo K] and the K loop runs three segments hi*hi, lo*hi, hi*lo.
// fp32 (one plane): a generic K-step is one tap of a 32-channel chunk, the interleaved layout's row with 32 fp32 in place of
// [32 hi | 32 lo].
struct ConvKLayout {
    ConvForm form;
    int kh, kw;       // the layer's kernel
    int kw_steps;     // kernel columns the K loop walks per row (kw; 1 where a K-step is a whole kernel row)
    int kstep;        // weight elements of one K-step per output channel (64; 32 fp32)
    int ck;           // channels of a generic layer's K-step (64; 32 interleaved or fp32)
    bool interleaved;
    int cchunks;      // channel chunks of ck (1 in the 4-channel forms)
    int ksteps_base;  // K-steps of one precision segment
    int Kbase;        // elements of one segment per weight row
    int Kw;           // weight row length in elements
    int nk;           // K-steps of the whole K loop
    int lo_at;        // the lo part of the weight at element k sits at k + lo_at
    // element of weight (ci, r, s) (hi part) in its row
    int index(int ci, int r, int s) const {
        if (form == CONV_FORM_STEM_ROWS) return r * 64 + s * 4 + ci;
        if (form == CONV_FORM_GENERIC) return (((ci / ck) * kh + r) * kw + s) * kstep + ci % ck;
        return r * (form == CONV_FORM_SMALL2 ? 4 : 8) * 4 + s * 4 + ci;
    }
};
// Cin: the activation's channel count (a multiple of 64, or 4 in the NHWC4 forms)
inline ConvKLayout conv_k_layout(int kh, int kw, int Cin, ConvForm form, wsc_precision prec) {
    ConvKLayout L;
    const int split = conv_split(prec);
    L.form = form; L.kh = kh; L.kw = kw;
    L.interleaved = split == 2 && conv_form_dma(form);
    L.kstep = prec == WSC_PREC_F32 ? 32 : 64;
    L.ck = (L.interleaved || prec == WSC_PREC_F32) ? 32 : 64;
    L.kw_steps = form == CONV_FORM_STEM_ROWS ? 1 : kw;
    L.cchunks = form == CONV_FORM_GENERIC ? Cin / L.ck : 1;
    if (form == CONV_FORM_GENERIC) L.ksteps_base = kh * kw * L.cchunks;
    else if (form == CONV_FORM_STEM_ROWS) L.ksteps_base = kh;
    else L.ksteps_base = (kh * (form == CONV_FORM_SMALL2 ? 4 : 8) * 4 + L.kstep - 1) / L.kstep;
    L.Kbase = L.ksteps_base * L.kstep;
    const bool segments = split != 0 && !L.interleaved;
    L.Kw = L.Kbase * (segments ? 2 : 1);
    L.nk = L.ksteps_base * (segments ? 3 : 1);
    L.lo_at = L.interleaved ? 32 : L.Kbase;
    return L;
}
// The IEEE-half modes store every output channel's weights times 2^shift, the power of two that puts the channel's largest |w|
// (`mx`) into [2^12, 2^13): mx = m 2^e with m in [0.5, 1) (frexp, fp32 denormals included), shift = 13 - e bounded to +-100 (a
// channel of ~1e-40 would otherwise ask for 2^(13 - e) = inf); a channel whose maximum is zero or not finite keeps shift 0.
// Integer arithmetic on the bits: the host packing (net.hip make_conv) and the device repack (repack.hip) get the same shift.
__host__ __device__ inline int conv_half_shift(float mx) {
    union { float f; uint32_t u; } v;
    v.f = mx;
    if (!(mx > 0.f) || (v.u & 0x7f800000u) == 0x7f800000u) return 0;
    const int E = (int)(v.u >> 23);
    const int e = E ? E - 126 : (31 - __builtin_clz(v.u)) - 148; // (denormal: M 2^-149, its top bit at 31 - clz)
    const int sh = 13 - e;
    return sh > 100 ? 100 : (sh < -100 ? -100 : sh);
}
// 2^sh as fp32, |sh| <= 126
__host__ __device__ inline float conv_pow2(int sh) {
    union { float f; uint32_t u; } v;
    v.u = (uint32_t)(sh + 127) << 23;
    return v.f;
}
// rows of the packed weights (and of scale / shift): whole 64-column tiles up to 64 channels, whole 128-column tiles beyond
inline int conv_cout_pad(int Cout) { return Cout <= 64 ? 64 : ((Cout + 127) / 128) * 128; }
// ... and the tile width the kernel takes for them
inline int conv_tile_bn(int CoutPad) { return CoutPad % 128 == 0 ? 128 : 64; }
// size of the zero-padded input of a CONV_FORM_STEM_ROWS layer: the rows the kernel rows of the last output pixel reach, an
// 8-pixel window per kernel row
inline void conv_stem_rows_input_dims(int Ho, int Wo, int stride, int kh, int *Hp, int *Wp) {
    *Hp = (Ho - 1) * stride + kh;
    *Wp = (Wo - 1) * stride + 8;
}

// The (mul, s1, s2) with which the conv kernels divide an unsigned n by d (d >= 1) without a division
inline void conv_fastdiv(unsigned d, unsigned *mul, unsigned *s1, unsigned *s2) {
    unsigned l = 0;
    while ((1ull << l) < d) ++l; // ceil(log2 d)
    *mul = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    *s1 = l < 1 ? l : 1;
    *s2 = l > 0 ? l - 1 : 0;
}

// One NHWC activation as host code passes it: its plane(s) and what they hold (16-bit values of conv_fmt(prec), or fp32 in
// WSC_PREC_F32).  In the two-plane precisions `lo` is a second plane of the same format and size.  The typed views are the
// only way to the values: the view of the other element type is a bug and aborts (a null Act has every view, null).
struct Act {
    void *hi = nullptr, *lo = nullptr; // lo: null in the one-plane precisions
    wsc_precision prec = WSC_PREC_BF16;
    explicit operator bool() const { return hi != nullptr; }
    int fmt() const { return conv_fmt(prec); }
    int split() const { return conv_split(prec); }
    // element `elems` of BOTH planes: THE place an element offset becomes a byte offset
    Act at(size_t elems) const {
        Act a = *this;
        a.hi = (char *)hi + elems * conv_elem_bytes(prec);
        if (lo) a.lo = (char *)lo + elems * conv_elem_bytes(prec);
        return a;
    }
    bool is_f32() const { return prec == WSC_PREC_F32; }
    bf16_t *h16() const { assert(!hi || !is_f32()); return (bf16_t *)hi; }
    bf16_t *h16_lo() const { assert(!hi || !is_f32()); return (bf16_t *)lo; }
    float *f32() const { assert(!hi || (is_f32() && !lo)); return (float *)hi; }
};
// Workspace layout of an activation of n elements: the hi plane, then (two-plane precisions) the lo plane, each a whole
// number of 256-byte lines.  act_carve hands the next one out at `cursor` and moves the cursor past it.
inline size_t act_bytes(size_t n, wsc_precision prec) {
    return (n * conv_elem_bytes(prec) + 255) / 256 * 256 * (conv_split(prec) ? 2 : 1);
}
inline Act act_carve(char *&cursor, size_t n, wsc_precision prec) {
    Act a;
    a.prec = prec;
    a.hi = cursor;
    if (conv_split(prec)) a.lo = cursor + act_bytes(n, prec) / 2;
    cursor += act_bytes(n, prec);
    return a;
}

// One conv layer as the kernel sees it.  Every activation operand has the layer's precision.
struct ConvLaunch {
    Act x;                      // input  [N][H][W][Cin]   (Cin = 4 in the NHWC4 forms)
    const void *w;              // packed [CoutPad][Kw]: conv_k_layout(kh, kw, Cin, form, prec); fp32 in WSC_PREC_F32, else 16-bit
    const float *s1, *b1;       // y = acc*s1 + b1 (folded BN, or conv bias with s1 = 1)
    const float *s2, *b2;       // optional post-ReLU affine (VGG's conv->ReLU->BN order), or null
    Act res;                    // optional residual [M][Cout]
    Act y;                      // output [M][Cout] (may be null when y_f32 is set)
    float *y_f32;               // optional fp32 output [M][Cout]
    int N, H, W, Cin, Ho, Wo, Cout, CoutPad;
    int kh, kw, stride, pad;
    int dil = 1;   // dilation, one rate for both axes: tap (r, s) of output pixel (ho, wo) reads input (ho * stride - pad + r * dil,
                   // wo * stride - pad + s * dil); > 1 on generic layers only (conv_igemm_launch sends them to the per-tap gather)
    int relu;
    ConvForm form;
    wsc_precision prec;
    int generic;   // 1: keep the generic kernel variants (testing: the FAST variants give the same bits)
    int ldy;       // row pitch of y in elements; 0 = Cout (wider: the output is a channel range of a concatenated tensor)
    // optional second input of a 1x1 / stride 1 layer: the last C2 of the Cin input channels of output pixel (n, ho, wo) come from
    // x2[n][ho * stride2][wo * stride2][0 .. C2) instead of x (which then holds Cin - C2 channels per pixel); null: one input
    Act x2;
    int H2, W2, C2, stride2;
    // every operand that is there holds values of `prec` (what the launchers check before they take the typed views)
    bool operands_match() const {
        for (const Act *a : {&x, &res, &y, &x2})
            if (*a && a->prec != prec) return false;
        return true;
    }
};
int conv_igemm_launch(wsc_ctx *ctx, const ConvLaunch &p);
// conv_f32.hip: the WSC_PREC_F32 layers (conv_igemm_launch sends them there)
int conv_f32_launch(wsc_ctx *ctx, const ConvLaunch &p);
// cam_head.hip: the 1x1 head with <= 32 output channels as a streaming GEMM (IEEE-half planes, fp32 [M][C] output)
int launch_cam_head(wsc_ctx *ctx, Act x, int M, int K, const bf16_t *w, int Kw, int CoutPad, const float *s1, const float *b1,
                    int C, int relu, float *y);

// ---- misc kernels ---------------------------------------------------------------------
// 1-D grid of a grid-stride kernel over `total` items (misc_kernels.hip, deeplab.hip, pool.hip; the files with a `grid_for` of
// their own cap theirs differently)
inline int wsc_grid_for(long long total, int block = 256, int cap = 256 * 16) {
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}
// The fp32 -> activation packs below are the doors of the range guard: with `range` = ctx->range_dev a value the planes cannot
// hold (NaN, +-inf; |v| >= 65504 in the IEEE-half formats) raises the ctx's range flag; null: no test (scratch that need not
// hold numbers, and the single-layer entries in the precisions that carry NaN / inf through: DESIGN.md section 5)
// (the single-layer entries: a door in the IEEE-half modes only)
inline unsigned *layer_door(wsc_ctx *ctx, wsc_precision prec) { return conv_fmt(prec) == 1 ? ctx->range_dev : nullptr; }
// (the kernel and its grid follow the activation's precision)
int launch_nchw_to_nhwc4(wsc_ctx *ctx, const float *x, int N, int H, int W, Act y, unsigned *range);
// stem_pool.hip: conv 7x7/2 + BN + ReLU + MaxPool 3x3/2/1 of the f16x3 ResNet stem in one kernel
void stem_pool_input_dims(int H, int W, int *Hp, int *Wp);
int launch_stem_pool(wsc_ctx *ctx, Act x, int N, int H, int W, const bf16_t *w, int Kw, const float *s1, const float *b1, int relu,
                     Act y);
// x[n][ho * stride][wo * stride][0 .. C) -> y[(n, ho, wo)][0 .. C) with row pitch ldy (both planes; y is at the first channel:
// Act::at(coff) of the wider tensor)
int launch_gather_strided(wsc_ctx *ctx, Act x, int N, int H, int W, int C, int stride, int Ho, int Wo, Act y, int ldy);
// [N][Hp][Wp][4] with a zero border of `pad` pixels on the top / left (and whatever Hp, Wp leave on the bottom / right)
int launch_nchw_to_nhwc4_pad(wsc_ctx *ctx, const float *x, int N, int H, int W, int Hp, int Wp, int pad, Act y, unsigned *range);
// cam[b][c][y][x] = relu(head[2b][y][x][c]) + relu(head[2b+1][y][w-1-x][c])   (head fp32 NHWC, stride Cs)
int launch_flip_add(wsc_ctx *ctx, const float *head, int B, int h, int w, int C, int Cs, float *cam);
// score[b][c] = sigmoid(sum_f mean_hw(feat[2b])[f] * Wc[c][f] + bias[c])
int launch_gap_linear_sigmoid(wsc_ctx *ctx, Act feat, int B, int hw, int F, const float *Wc, const float *bias, int C, float *score,
                              int sample_stride);
// y[i] = the fp32 value of activation element i (hi + lo in the two-plane precisions), i < n
int launch_act_to_f32(wsc_ctx *ctx, Act x, size_t n, float *y);
int launch_nchw_to_nhwc(wsc_ctx *ctx, const float *x, int N, int C, int HW, Act y, unsigned *range);
int launch_nhwc_to_nchw(wsc_ctx *ctx, Act x, int N, int C, int HW, float *y);

// ---- pool.hip: every K x K pooling window on an NHWC activation ----------------------------------------------------------------
// How (out, pad_before) of an axis follow from (in, k, stride) -- THE statement of the three rules (wsscam/net/common.py::
// pool_axis is the Python side's):
//   POOL_TORCH     nn.MaxPool2d(k, stride, pad): out = (in + 2 pad - k) / stride + 1, pad_before = pad
//                  (C division: an axis less than `stride` short of the padded window keeps one window, the part of it inside
//                  the image -- the nets always sized their pools so; wsc_maxpool_nhwc rejects such a map itself)
//   POOL_TF_SAME   out = ceil(in / stride), pad_before = max((out - 1) stride + k - in, 0) / 2 (floor; the rest after: 1 / 1 on an
//                  odd size, 0 / 1 on an even size at 3 x 3 / 2 -- what one symmetric pad cannot express)
//   POOL_TF_VALID  out = (in - k) / stride + 1, no padding
enum PoolRule { POOL_TORCH, POOL_TF_SAME, POOL_TF_VALID };
struct PoolGeom {
    int k, stride, pad_t, pad_l, Ho, Wo;
    bool avg; // the average over the in-image taps instead of their maximum
};
inline bool pool_axis(PoolRule rule, int in, int k, int stride, int pad, int *out, int *pad_before) {
    *out = *pad_before = 0;
    if (in < 1 || k < 1 || stride < 1) return false;
    if (rule == POOL_TF_SAME) {
        *out = (in + stride - 1) / stride;
        const int pad_total = (*out - 1) * stride + k - in;
        *pad_before = pad_total > 0 ? pad_total / 2 : 0;
    } else if (rule == POOL_TF_VALID) {
        *out = in >= k ? (in - k) / stride + 1 : 0;
    } else {
        if (pad < 0) return false;
        *pad_before = pad;
        *out = (in + 2 * pad - k) / stride + 1;
    }
    return *out >= 1;
}
// false (and nothing to launch) when H x W is no input of that window: an axis shorter than the (padded) window
inline bool pool_geom(PoolRule rule, int k, int stride, int pad /* POOL_TORCH only */, bool avg, int H, int W, PoolGeom *g) {
    g->k = k; g->stride = stride; g->avg = avg;
    const bool okh = pool_axis(rule, H, k, stride, pad, &g->Ho, &g->pad_t), okw = pool_axis(rule, W, k, stride, pad, &g->Wo, &g->pad_l);
    return okh && okw;
}
// max (padding never wins) or average (k = 3, stride 1) of that geometry, every plane; the kernel follows the activation's precision
int launch_pool(wsc_ctx *ctx, Act x, int N, int H, int W, int C, const PoolGeom &g, Act y);

// the gradient of launch_pool with respect to its input (fp32 planes): dx[n][hi][wi][c] = the sum, in window order, of dy over the
// windows whose first maximum (row-major window order, recomputed from x) is that pixel -- or of dy / (in-image tap count) over
// the windows that cover it (g.avg).  Gather form: no atomics.  C a multiple of 4.
int launch_pool_grad(wsc_ctx *ctx, const float *x, const float *dy, int N, int H, int W, int C, const PoolGeom &g, float *dx);

// ---- seg_grad.hip: the fp32 kernels of the DeepLab backward pass -------------------------------------------------------------
// How one layer's weight gradient is cut into blocks (wgrad_plan) -- what its caller sizes the slabs by
struct WgradPlan {
    int M, nk, pad;             // pixels, K-steps of 32 pixels, SAME padding
    bool small_cin;             // Cin = 3: the (tap, channel) pairs as one 32-row operand
    int bn, tiles_ci, tiles_co; // column tile (32 / 64 / 128), 64-row and bn-column tiles
    int ntaps;                  // taps that get blocks
    unsigned long long taps;    // their r k + s, 4 bits each
    unsigned dead;              // bit r k + s: the tap is outside the image for every pixel (exact zeros, nothing read)
    int splits;                 // K slices
    long long out_elems, slab_elems; // k k Cin Cout; floats of the split-K slabs
};
// splits = 0: the launcher's choice (blocks ~ 1 - 2 x the CU count); Cin 3 or a multiple of 64, Cout 2 .. 32 or a multiple of 64
int wgrad_plan(const wsc_ctx *ctx, int N, int H, int W, int Cin, int Cout, int k, int dil, int splits, WgradPlan *pl);
// dw [k][k][Cin][Cout] (HWIO) of a stride-1 SAME convolution from x [N][H][W][Cin] and dz [N][H][W][Cout]; every element is written
int wgrad_launch(wsc_ctx *ctx, const WgradPlan &pl, const float *x, const float *dz, int H, int W, int Cin, int Cout, int k, int dil,
                 float *slab, float *dw);
// dz = dy scale [y > 0], the product one fp32 rounding (scale 1.0f: dy itself, bit for bit; > 1 behind a dropout site, whose tape
// entry is > 0 exactly where the unit was kept and its ReLU positive); y null: dz = dy, no scale; dz null: not written;
// db[c] = sum_m dz[m][c]; partial: relu_bias_grad_blocks(M) * C floats
int relu_bias_grad_blocks(long long M);
int launch_relu_bias_grad(wsc_ctx *ctx, const float *y, const float *dy, long long M, int C, float scale, float *dz, float *partial,
                          float *db);
// dst [M][Cd] = the first channels of src [M][Cs], zeros beyond
int launch_copy_channels(wsc_ctx *ctx, const float *src, long long M, int Cs, int Cd, float *dst);
// The data gradient of a stride-1 SAME convolution w [k][k][Cin][Cout] as conv_f32_launch's generic layer: its input is dz with
// dgrad_cz(Cout) channels (zeros past Cout), its kernel the rotated, transposed one in conv_k_layout(k, k, dgrad_cz(Cout), generic,
// WSC_PREC_F32) with conv_cout_pad(Cin) rows; ones / zeros: that many 1.0 / 0.0.  sum_with: null, or [M][Cin] added to the result
// (may be dx itself: every element is read and written by one thread).
inline int dgrad_cz(int Cout) { return (Cout + 31) / 32 * 32; }
void dgrad_pack(const float *w_hwio, int k, int Cin, int Cout, std::vector<float> *packed);
int dgrad_launch(wsc_ctx *ctx, const float *dz, const float *w_packed, const float *ones, const float *zeros, int N, int H, int W, int Cin,
                 int Cout, int k, int dil, const float *sum_with, float *dx);

// whether a launch may take the 16-byte forms of its loads and stores on `p`
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- sgd.hip: the optimiser steps of the three training paths, each on the flat fp32 parameter layout of its gradient object
// (the contract: its header); every product, sum and quotient one fp32 rounding ----------------------------------------------------
// SEC / DSRG, the layout of wsc_seg_grad_layout.  One run of floats of that layout with one learning-rate multiplier: a layer's w
// (decay = 1: the weight-decay term applies and the floats count into loss["l2"]) or its b.  The table has a segment per run in
// offset order; the kernel finds an element's segment itself, so the offsets may be any (odd ones included).
struct SgdSegment {
    long long start; // first float
    float mult;      // 1 / 2 (bias) / 10 (fc8 w) / 20 (fc8 b)
    int decay;
};
constexpr int SGD_MAX_SEGMENTS = 128;  // (a DSRG net has 50)
constexpr int SGD_L2_MAX_BLOCKS = 1024; // blocks of the accumulate kernel = doubles of `l2_partials`
// accum += mult (grad [+ wd param]) / accum_num; l2_dev (or null) = sum w^2 / 2 over the decay segments, summed in double in a
// fixed order (l2_partials: SGD_L2_MAX_BLOCKS doubles, l2_counter: one unsigned, both the caller's and used by one stream)
int sgd_accumulate_launch(wsc_ctx *ctx, const SgdSegment *segs_dev, int n_segs, const float *param, const float *grad, float *accum,
                          long long elems, float weight_decay, int accum_num, double *l2_partials, unsigned *l2_counter, float *l2_dev);
// mom = mom momentum + accum, param -= lr mom (TensorFlow's ApplyMomentum, use_nesterov = False); clear_accum: accum = +0.0
int sgd_apply_launch(wsc_ctx *ctx, float *param, float *accum, float *mom, long long elems, float lr, float momentum, int clear_accum);
// IRNet, the layout of wsc_irn_grad_layout: g = grad + wd p; m = momentum m + g; p = p - lr m with lr = lr_a for the elements
// before `boundary`, lr_b from there on; grad is only read
int irn_sgd_launch(wsc_ctx *ctx, float *param, const float *grad, float *mom, long long elems, long long boundary, float lr_a, float lr_b,
                   float weight_decay, float momentum);
// 01_train, the layout of wsc_cls_param_layout: v = momentum m - lr g; m = v; p = (p + momentum v) - lr g (nesterov) / p + v; lr g
// formed once; grad is only read
int cls_sgd_launch(wsc_ctx *ctx, float *param, const float *grad, float *mom, long long elems, float lr, float momentum, int nesterov);

// ---- repack.hip: the updated floats of a parameter buffer into a net, what the three wsc_net_*_load_params launch (the
// contract: its header).  Each launch below serves every job of a device table: a job carries its first block in that launch, jobs
// in order, the block offsets non-decreasing (an empty range: no blocks); a kernel finds its block's job there ----------------------
// The conv rows: a layer's weights w [k][k][Cin][Cout] (HWIO) and bias b [Cout], at their offsets of the flat parameter buffer,
// into everything derived from them -- the packed rows `wp` [CoutPad][Kw] of conv_k_layout(k, k, Cin or 4, form, prec) with
// s1 / b1, the bytes make_conv gives, and (w_rot non-null) the rotated, channel-transposed fp32 kernel of dgrad_pack.
// One RepackJob per layer in a device table built once per gradient object: the caller fills the layer's fields, repack_plan adds
// the layout, the split of the channel maxima and where the layer's blocks lie in each of the (at most four) launches of a repack.
struct RepackJob {
    long long w_off, b_off;          // floats into the parameter buffer; b_off < 0: no bias, b1 = 0 (the IRNet heads)
    int k, Cin, Cout;                // Cin as in the HWIO tensor (3 for the first layer)
    int Cin_pad;                     // 0, or the channels of the layer's INPUT where it is wider than the tensor (the final edge conv
                                     // of IRNet: 160 in 192); the packed rows hold exact zeros for the channels past Cin
    int small;                       // CONV_FORM_SMALL2 (the first layer), else CONV_FORM_GENERIC
    int kstep, Kw, lo_at, nsteps;    // conv_k_layout; nsteps: the K-steps of one precision segment
    int rot_Kw;                      // k k dgrad_cz(Cout), the row of the rotated kernel; 0 without one
    int splits, rows_per;            // partial channel maxima (IEEE-half modes, generic layers): row ranges of rows_per rows
    int max_block0, pack_block0, rot_block0; // the layer's first block in the maxima / pack / rotate launch
    int tiles;                       // 64-channel column tiles
    long long pmax_off;              // floats into the scratch of the partial maxima
    void *wp;
    float *s1, *b1, *w_rot;
};
struct RepackPlan {
    RepackJob *jobs_dev = nullptr;
    int n_jobs = 0, small_job = -1, small_tiles = 0;
    int ck = 0; // channels of a generic layer's K-step (conv_k_layout)
    int max_blocks = 0, pack_blocks = 0, rot_blocks = 0;
    long long pmax_elems = 0;
    float *pmax = nullptr;
    wsc_precision prec = WSC_PREC_BF16;
    double bytes = 0; // algorithmic traffic of one repack
};
int repack_plan(std::vector<RepackJob> &jobs, wsc_precision prec, RepackPlan *plan);
int repack_launch(wsc_ctx *ctx, const RepackPlan &plan, const float *param);
// One run of floats of the parameter buffer that a repack copies as it is (GroupNorm weight / bias of a head)
struct VecCopyJob {
    long long off; // floats into the parameter buffer
    int n, block0; // its length; the job's first block in the launch
    float *dst;
};
constexpr int VEC_COPY_PER_BLOCK = 256;
// (block0 filled by the caller: ceil(n / VEC_COPY_PER_BLOCK) blocks each)
int vec_copy_launch(wsc_ctx *ctx, const VecCopyJob *jobs_dev, int n_jobs, int blocks, const float *param);
// One BatchNorm layer's inference epilogue: s2[c] = float(gamma / sqrt(var + eps)), b2[c] = float(beta - mean sc) in double, from
// gamma / beta at their offsets of the parameter buffer and the layer's [2][C] block of the running statistics
struct BnFoldJob {
    long long g_off, be_off, run_off; // floats into the parameter buffer (gamma, beta) / the running statistics (mean; var C floats on)
    int C, block0;                    // channels; the job's first block in the launch
    double eps;                       // as fold_bn of net.hip takes it
    float *s2, *b2;
};
constexpr int BN_FOLD_PER_BLOCK = 256;
// (block0 filled by the caller: ceil(C / BN_FOLD_PER_BLOCK) blocks each)
int bn_fold_launch(wsc_ctx *ctx, const BnFoldJob *jobs_dev, int n_jobs, int blocks, const float *param, const float *run);
// dst [F][C] = the transpose of src [C][F] (the classifier's Linear, torch's layout, as the conv rows read it)
int transpose_cf_launch(wsc_ctx *ctx, const float *src, int C, int F, float *dst);

// ---- seg_dropout.hip: the dropout sites behind fc6 / fc7 of the SEC / DSRG training graph (the contract: its header) -----------
// WSC_ERR_INVALID unless 0 <= drop_prob < 1 (NaN included) and 0 <= step < 2^32; `fn` names the caller in the error text
int seg_dropout_check(const char *fn, float drop_prob, long long step);
// 1 / (1 - drop_prob) in fp32: the forward kernel's factor and the backward pass's
float seg_dropout_scale(float drop_prob);
// y[i] = dropout of x[i] (y may be x) with element i at index first + i of the logical tensor; tape (fp32 copy of y) and keep (one
// byte per element) are optional
int launch_seg_dropout_f32(wsc_ctx *ctx, const float *x, float *y, float *tape, uint8_t *keep, long long n, unsigned long long first,
                           float drop_prob, unsigned long long seed, unsigned step, unsigned site);
// the activation's n elements in place, every precision; tape (or null) receives the fp32 value the planes hold afterwards (in
// place of launch_act_to_f32); Cout: what the range flag is raised with where an IEEE half reaches the ceiling
int launch_seg_dropout(wsc_ctx *ctx, Act a, size_t n, int Cout, float drop_prob, unsigned long long seed, unsigned step, unsigned site,
                       float *tape);

// ---- deeplab.hip: the kernels around the conv stack of the SEC / DSRG DeepLab nets -------------------------------------
// float32 [N][H][W][3] -> NHWC4 activation (raises the range flag where an IEEE-half plane saturates)
int launch_nhwc3_to_nhwc4(wsc_ctx *ctx, const float *x, int N, int H, int W, Act y);
// prob[m][c] = fc8-softmax of (in[0] + ... + in[n_in - 1])[m][c]; fc8 (optional) receives the summed logits
int launch_fc8_softmax(wsc_ctx *ctx, const float *const *in, int n_in, long long M, int C, float min_prob, float *fc8, float *prob);

// ---- seg_eval.hip / seg_chain.hip: the SEC / DSRG prediction loop around the dense CRF ------------------------------------
constexpr int SEG_MAX_C = 32; // the class limit of wsc_crf_v_inference, whose unaries / marginals these files handle

// ---- irn_kernels.hip ---------------------------------------------------------------------
int launch_group_norm_stats(wsc_ctx *ctx, const float *x, int N, int H, int W, int C, int G, float eps, void *partial,
                            void *stats);
size_t group_norm_partial_bytes(int N, int H, int W, int G);
// y: the whole [N][Hd][Wd][Ctot] concat tensor; this head writes its channels [coff, coff + C)
int launch_group_norm_apply(wsc_ctx *ctx, const float *x, const void *stats, const float *gamma, const float *beta,
                            int N, int H, int W, int C, int G, int up, int relu, Act y, int Hd, int Wd, int Ctot, int coff);
int launch_edge_finish(wsc_ctx *ctx, const float *e, int He, int We, const float *d, int Hd, int Wd, int B, int fh, int fw,
                       float ms0, float ms1, float *edge, float *dp);
// e [N][He][We], d [N][Hd][Wd][2] (8-byte aligned) -> edge [N][He][We], dp [N][2][Hd][Wd]
int launch_edge_raw(wsc_ctx *ctx, const float *e, int He, int We, const float *d, int Hd, int Wd, int N, float *edge, float *dp);

// ---- irn_grad.hip: the fp32 / double kernels of the backward pass of the IRNet heads and the channel mean of the closing dp_mean
// pass (the contract: its header) ---------------------------------------------------------------------------------------------
// dy [N][H][W][C] = the adjoint of "upsample by `up`, crop to Hd x Wd, ReLU, write channels [coff, coff + C)" applied to dcat
// [N][Hd][Wd][Ctot]; the ReLU mask is cat > 0 (the taped concat values); every element of dy is written
int launch_relu_upsample_grad(wsc_ctx *ctx, const float *dcat, const float *cat, int N, int H, int W, int C, int up, int Hd, int Wd, int Ctot,
                              int coff, float *dy);
// dz [N][H][W][C], dgamma [C], dbeta [C] of GroupNorm(G, C) from its input z, the {mean, rstd} pairs `stats` [N][G] of the forward
// pass and the gradient dy of its output; partial: group_norm_grad_partial_bytes, ms: N G double2
size_t group_norm_grad_partial_bytes(int N, int H, int W, int C);
int launch_group_norm_grad(wsc_ctx *ctx, const float *z, const void *stats, const float *gamma, const float *dy, int N, int H, int W, int C,
                           int G, void *partial, void *ms, float *dz, float *dgamma, float *dbeta);
// y [N][Ho][Wo][C] = x[:, ::stride, ::stride, :] (C a multiple of 4)
int launch_strided_rows_f32(wsc_ctx *ctx, const float *x, int N, int H, int W, int C, int stride, int Ho, int Wo, float *y);
// ddp [N][2][HW] -> out [N HW][Cd], zeros past channel 1
int launch_dp_to_nhwc(wsc_ctx *ctx, const float *ddp, int N, int HW, int Cd, float *out);
// out[c] (device doubles) = mean over (n, p) of x[n][c][p] in double, minus sub_host[c] (floats, or null); the scratch (tickets,
// partials, the uploaded sub) is one cached block of the ctx, handed back behind the launch
constexpr int CHANNEL_MEAN_MAX_BLOCKS = 64; // per channel
constexpr int CHANNEL_MEAN_MAX_C = 1024;
int channel_mean_launch(wsc_ctx *ctx, const float *x, int N, int C, long long HW, const float *sub_host, double *out);

// ---- cls_grad.hip: BatchNorm in training mode on a [M][C] fp32 matrix (the contract: its header and include/wsscam.h) -----------
// stats [C] float {mean, rstd} pairs of the batch; run: null, or [2][C] running mean / variance updated in place with `keep` the
// weight of the old value; y (or null: the statistics alone) = fma((a - mean) rstd, gamma, beta), gn_affine's expression.  The
// scratch is a cached block of the ctx.  C a multiple of 4 up to 1024, M < 2^31
int launch_batch_norm_train(wsc_ctx *ctx, const float *a, long long M, int C, const float *gamma, const float *beta, float eps, float keep,
                            int unbiased, float *run, float *stats, float *y);
// da [M][C], dgamma [C], dbeta [C] from the input a, the forward pass's float statistics and the gradient dy of the output
int launch_batch_norm_grad(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *dy, long long M, int C,
                           float *da, float *dgamma, float *dbeta);
// A dropout site behind a BatchNorm (dropout_rng.h's contract; the caller has checked drop_prob and step: seg_dropout_check).
// Forward: y = fma((a - mean) rstd, gamma, beta) from the stats launch_batch_norm_train left, dropped and scaled in fp32, stored
// ONCE into `act` (any precision; the GroupNorm store's split and range flag) and, as the fp32 value `act` then holds, into tape
// (or null) -- in place of launch_group_norm_apply + launch_act_to_f32.  16-byte accesses where gamma, beta, act and tape allow,
// else the scalar form: the same bits
int launch_batch_norm_apply_drop(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *beta, long long M, int C,
                                 Act act, float *tape, float drop_prob, unsigned long long seed, unsigned step, unsigned site);
// Backward: launch_batch_norm_grad with dy the gradient BEHIND the dropout -- the kernels replace it on load by
// keep ? fmul_rn(dy, scale) : +0.0 with the keep bits regenerated from (seed, step, site)
int launch_batch_norm_grad_drop(wsc_ctx *ctx, const float *a, const float *stats, const float *gamma, const float *dy, long long M, int C,
                                float *da, float *dgamma, float *dbeta, float drop_prob, unsigned long long seed, unsigned step, unsigned site);

