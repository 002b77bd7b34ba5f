/*
 * wsscam.h -- C ABI of libwsscam, the MI355X (gfx950) implementation of the
 * CAM pseudo-label hot path of lyndonchan/wsss-analysis.
 *
 * The reference has no FFI for this path: it is Python calling torch / Keras /
 * cv2 / pydensecrf.  Each entry point below names the reference code it
 * replaces (file:line under the reference tree).  The Python shim in
 * wsss-analysis_amd/wsscam binds exactly these symbols with ctypes and keeps
 * the reference's Python signatures and on-disk formats on top of them.
 *
 * Conventions
 *   - every function returns 0 (WSC_OK) or a negative wsc_status; nothing
 *     throws, nothing calls exit().  wsc_last_error() returns a thread-local
 *     message for the last failing call on this thread.
 *   - all data pointers named *_dev are DEVICE pointers (hipMalloc'ed memory,
 *     e.g. torch.Tensor.data_ptr() or wsc_malloc); pointers named *_host are
 *     host pointers.  The caller owns every buffer it passes in; the library
 *     owns only what a wsc_*_create returned.
 *   - a wsc_ctx is bound to one device and one HIP stream.  All work of a ctx
 *     is enqueued on that stream and is asynchronous unless stated; wsc_sync
 *     waits for it.  Distinct ctxs may be used from distinct threads.
 *   - there is no CPU fallback: if no gfx950 device is present
 *     wsc_ctx_create fails with WSC_ERR_NO_DEVICE.
 */
#ifndef WSSCAM_H
#define WSSCAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSC_VERSION 100 /* 0.1.0 */

typedef enum wsc_status {
    WSC_OK = 0,
    WSC_ERR_INVALID = -1,     /* bad argument (shape, null pointer, enum) */
    WSC_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture */
    WSC_ERR_HIP = -3,         /* a HIP runtime call failed */
    WSC_ERR_MISSING_KEY = -4, /* state-dict key missing (strict load) */
    WSC_ERR_SHAPE = -5,       /* state-dict tensor has the wrong shape */
    WSC_ERR_NOMEM = -6,
    WSC_ERR_KEY_RANGE = -7,   /* CRF lattice coordinate outside packed-key range */
    WSC_ERR_CAPACITY = -8,    /* CRF hash table / vertex capacity exceeded */
    WSC_ERR_RANGE = -9        /* an activation of an IEEE-half mode (f16, f16x3) left half's finite range (|v| >= 65504) and was
                                 saturated: the reference's fp32 (03b_irn/net/resnet50.py:11-14) has no such ceiling, so the maps
                                 of this ctx are NOT the reference's.  Sticky: returned by wsc_sync / wsc_memcpy_d2h until
                                 wsc_ctx_range_status(ctx, &f, 1) clears it.  Run the model in WSC_PREC_F32, the exact fallback, instead
                                 (WSC_PREC_BF16X3 also has fp32's range, with a 16-bit significand).
                                 NaN and inf: a non-finite element given to a network-path entry point is either LOUD -- this
                                 status from the call, with a text that names the cause (a non-finite state-dict tensor at
                                 wsc_net_create, a non-finite weight / scale / shift of an IEEE-half layer), or the same sticky flag,
                                 raised by the fp32 -> activation packs, the device repack and the GroupNorm store -- or it
                                 PROPAGATES: every cell that is non-finite in the reference is non-finite on the device.  Never a
                                 plausible finite map.  Which one per entry point and precision: DESIGN.md section 5, "NaN and
                                 inf".  Every whole-net forward and every IEEE-half entry is loud; the single-layer entries in
                                 bf16 / bf16x3 / f32, the fp32 gradient kernels, wsc_cls_loss and the SGD steps propagate */
} wsc_status;

/* architectures: 03b_irn/net/{resnet50_cam,vgg16_cam,m7_cam}.py */
typedef enum wsc_arch {
    WSC_ARCH_RESNET50_CAM = 0, /* net/resnet50.py:57-108 + resnet50_cam.py:12-20,55-70 */
    WSC_ARCH_VGG16_CAM = 1,    /* net/vgg16.py:44 + common_cnn.py:128-141 + vgg16_cam.py:24-60 */
    WSC_ARCH_M7_CAM = 2,       /* net/m7.py:41 + m7_cam.py:22-57 */
    WSC_ARCH_RESNET50_IRN = 3, /* net/resnet50_irn.py:8-132,210-232 (EdgeDisplacement) */
    WSC_ARCH_VGG16_IRN = 4,    /* net/vgg16_irn.py:8-212,301-321 (EdgeDisplacement, ds_fac = 0.25) */
    WSC_ARCH_M7_IRN = 5,       /* net/m7_irn.py:8-118,195-213 (EdgeDisplacement; edge map at 1/2 resolution) */
    WSC_ARCH_DEEPLAB_LFOV = 6, /* 03a_sec-dsrg/SEC.py:117-128,150-218: DeepLab-VGG16, one fc6 / fc7 / fc8 branch at rate 12 */
    WSC_ARCH_DEEPLAB_ASPP = 7  /* 03a_sec-dsrg/DSRG.py:169-186,203-295: the same trunk, branches _1 .. _4 at rates 6 / 12 / 18 / 24,
                                  fc8 = their sum */
} wsc_arch;

/* arithmetic of the conv stack */
typedef enum wsc_precision {
    WSC_PREC_BF16 = 0,  /* bf16 operands, fp32 MFMA accumulation, bf16 activations in HBM */
    WSC_PREC_BF16X3 = 1, /* split-bf16 (hi+lo) operands, 3 MFMA products: fp32-class accuracy */
    WSC_PREC_F16 = 2,    /* IEEE half operands (11-bit significand, saturating), fp32 accumulation */
    WSC_PREC_F16X3 = 3,  /* split-half (hi+lo, 22-bit significand) operands and activations, 3 MFMA products per K-slice with
                            both planes staged once: the fp32-class mode (reference arithmetic is fp32, SURVEY 8 header) */
    WSC_PREC_F32 = 4     /* exact fp32: fp32 weights and activations, fp32-input MFMA (an fmaf chain), no range guard needed --
                            the reference's arithmetic and range, the fallback for WSC_ERR_RANGE */
} wsc_precision;

typedef struct wsc_ctx wsc_ctx; /* device + stream + workspace arena */
typedef struct wsc_net wsc_net; /* immutable packed weights of one CNN */
/* Path selectors of a context (wsc_ctx_set_option).  Each one chooses between two code paths that BOTH serve some inputs
 * in the default configuration (e.g. the Gaussian message is formed on chip only while a tile's vertex set fits the LDS) and
 * are held to identical bits by tests/test_gpu_crf.py and tests/test_gpu_irn.py; the selector forces the fallback for every
 * input so that a test (or a debugging session) can compare.  There are no environment switches in the library. */
typedef enum {
    WSC_OPT_CRF_GAUSS_ON_CHIP = 0, /* default 1; 0: blur kernels + value-row gathers instead of gauss_msg_kernel */
    WSC_OPT_CRF_FUSED_BLUR = 1,    /* default 1; 0: three blur4 passes instead of blur3_tile_kernel (Gaussian lattice) */
    WSC_OPT_CRF_BLUR_ON_CHIP = 2,  /* default 1; 0: one blur4 launch per pass instead of blur_lds_kernel (bilateral lattice) */
    WSC_OPT_CRF_RANK_BALLOT = 3,   /* default 0; 1: ballot-matching rank walk for every tile of the lattice build */
    WSC_OPT_CRF_EMBED_FULL = 4,    /* default 0; 1: the 2048-slot LDS table for every tile of the lattice build */
    WSC_OPT_RW_TILED = 5,          /* default -1 (by batch size); 0: flat random-walk step; 1: tiled step */
    WSC_OPT_STEM_POOL_FUSED = 6,   /* default 1; 0: the f16x3 ResNet stem as conv_igemm + max-pool launches instead of stem_pool_kernel */
    WSC_OPT_CONV_WINDOW = 7,       /* default 1; 0: per-tap A tiles instead of the LDS input window of the f16x3 3x3 / stride 1 layers (same bits) */
    WSC_OPT_CAM_HEAD_STREAM = 8,   /* default 1; 0: the 1x1 CAM / Grad-CAM head through the tiled conv kernel instead of cam_head_kernel
                                      (the one selector whose two paths are equal to fp32 round-off, not bit-identical: K is summed in four quarters) */
    WSC_OPT_CRF_MSG_IN_UPDATE = 9, /* default 1; 0: gauss_msg_kernel + update_splat_kernel as two launches with E = -U + Gaussian message in HBM between
                                      them, instead of the message formed inside the update kernel (same bits) */
    WSC_OPT_COUNT = 10
} wsc_option;

typedef struct wsc_crf wsc_crf; /* lattices (Gaussian + bilateral) of a batch of images */
typedef struct wsc_crf_v wsc_crf_v; /* the same for a RAGGED batch: every image its own (H, W) and class count */

/* A named host tensor of a torch state_dict (float32, C-contiguous). */
typedef struct wsc_tensor_desc {
    const char *name;  /* e.g. "resnet50.layer1.0.conv1.weight" */
    const float *data; /* host pointer */
    int32_t ndim;
    int64_t shape[4];
} wsc_tensor_desc;

/* ---- library / context ------------------------------------------------ */

int wsc_version(void);
const char *wsc_last_error(void);

/* device: HIP device ordinal.  stream: a hipStream_t to enqueue on (e.g.
 * torch.cuda.current_stream().cuda_stream), or NULL to let the ctx create and
 * own a stream.  Replaces `model.cuda()` / `cuda.device(process_id)`
 * (03b_irn/step/make_cam.py:31-33). */
int wsc_ctx_create(int device, void *stream, wsc_ctx **out);
void wsc_ctx_destroy(wsc_ctx *ctx);
/* Sets a path selector (wsc_option) of the context; WSC_ERR_INVALID for an unknown option. */
int wsc_ctx_set_option(wsc_ctx *ctx, int option, int value);
/* Test hook for the scratch contract: scratch holds arbitrary bits on entry, and whatever a kernel reads, a kernel or
 * memset of the same call wrote.  value 0..255 sets the context's fill byte, -1 turns the fill off (the default); anything else is
 * WSC_ERR_INVALID (the hook then stays as it was, as after a failed fill).  On the call the workspace arena and every block on
 * the cached allocator's free list are set to the byte, in stream order; while it is on, every cached block handed out (fresh or
 * reused) and the WHOLE arena at every request of an entry point (no entry keeps arena contents across a request) are set to it
 * before the caller gets them; so are the private workspaces of a wsc_seg_grad / wsc_irn_grad at the start of every backward or
 * load_params call (nothing in them outlives a call).  Live blocks (weights, lattices, the Gaussian-lattice cache) and caller
 * buffers are never touched.
 * Not a wsc_option: results must not depend on it at all, which tests/test_gpu_scratch.py checks.  Off: no launch, no sync. */
int wsc_ctx_scratch_fill(wsc_ctx *ctx, int value);
/* The hook's current value: -1 (off) or the fill byte. */
int wsc_ctx_scratch_fill_value(const wsc_ctx *ctx);
int wsc_sync(wsc_ctx *ctx);
/* Range guard of the IEEE-half conv modes.  Every conv epilogue that writes half activations raises a sticky per-ctx flag when
 * a value reaches the half ceiling (it is stored saturated at +-65504; fp32 in the reference would have kept it).  wsc_sync and
 * wsc_memcpy_d2h report the raised flag as WSC_ERR_RANGE AFTER completing their work (the copy is done, the stream is idle).
 * *flag_out (may be NULL): 0 = clean, otherwise the output-channel count of a layer that saturated.  Synchronises the ctx
 * stream.  clear != 0 resets the flag. */
int wsc_ctx_range_status(wsc_ctx *ctx, int *flag_out, int clear);
/* Make all work enqueued on `ctx` after this call wait (on the device, without blocking the host) for
 * everything enqueued so far on `other`: lets one process overlap independent stages on two contexts
 * of the same device (e.g. the lattice build of a batch, which needs only the RGB images, with its
 * CNN forward pass) and join them before the stage that needs both. */
int wsc_ctx_wait(wsc_ctx *ctx, wsc_ctx *other);
/* Markers: wsc_ctx_mark records marker `slot` (0 .. 7) at the current end of the ctx's stream; wsc_ctx_wait_mark blocks the
 * HOST until everything enqueued before that record has completed (and returns at once for a slot never recorded).  A caller
 * that keeps several steps in flight on one stream waits for "the step two back" this way -- without a wsc_sync that would
 * also wait for the newest one, and without an extra stream whose wait packets can end up in front of another stream's
 * kernels on a shared hardware queue (replaces the `torch.cuda.synchronize()` granularity of 03b_irn/step/make_cam.py:81-85). */
int wsc_ctx_mark(wsc_ctx *ctx, int slot);
int wsc_ctx_wait_mark(wsc_ctx *ctx, int slot);
/* Device-side: work enqueued on `ctx` after this call waits for marker `slot` of `other` (its last record) -- and for nothing
 * `other` enqueued after that record, unlike wsc_ctx_wait.  No-op for a slot never recorded.  Same device. */
int wsc_ctx_wait_for_mark(wsc_ctx *ctx, wsc_ctx *other, int slot);
/* name of the device's gcnArchName ("gfx950...") and CU count */
int wsc_device_info(wsc_ctx *ctx, char *arch_name, size_t arch_name_len, int *num_cus);

/* device memory helpers so a host without torch can drive the library
 * (replace tensor.cuda() / .cpu(): make_cam.py:48,81-82) */
int wsc_malloc(wsc_ctx *ctx, size_t bytes, void **dptr_out);
int wsc_free(wsc_ctx *ctx, void *dptr);
int wsc_memcpy_h2d(wsc_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes); /* async on ctx stream */
int wsc_memcpy_d2h(wsc_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* synchronises */
int wsc_memset(wsc_ctx *ctx, void *dst_dev, int value, size_t bytes);
/* Page-locked host staging for the batch pipeline (replaces DataLoader(pin_memory=...) + .cuda(non_blocking=True),
 * make_cam.py:29,45-48, and the .cpu() copies of :81-85): copies between pinned memory and the device are truly
 * asynchronous on the ctx stream; the host buffer must stay untouched until a later wsc_sync(ctx) returns. */
int wsc_host_alloc(wsc_ctx *ctx, size_t bytes, void **host_out);
int wsc_host_free(wsc_ctx *ctx, void *host);
/* Host I/O helper of the writer threads (03b_irn/step/make_cam.py:80-88 np.save per image): creates / truncates `path` and
 * writes the n byte segments one after the other (open + writev + close; no GPU involved, any thread).  A caller that holds
 * the bytes of an .npy container as [header | metadata | array | metadata | array ...] writes the arrays straight from where
 * they are (e.g. the page-locked staging buffer of a D2H copy) without the interpreter lock: wsscam.step.make_cam.save_npy_object. */
int wsc_host_write_segments(const char *path, int n, const void *const *ptrs, const size_t *sizes);
/* Asynchronous copies on the context's stream (page-locked host memory).  Scheduling note for callers with several contexts in
 * flight: the runtime hands a queued copy to a DMA engine at once and turns "after the kernels before it on the stream" into a
 * poll command on that engine's in-order queue -- every copy submitted later to the same engine, from ANY context, waits behind
 * it.  Issue a copy when its producers have (nearly) finished: wsc_ctx_mark after the producer, wsc_ctx_wait_mark on a helper
 * thread, then the copy (bench.py's end-to-end leg, wsscam.step.pipeline._copy_out); wsc_memcpy_d2h does that wait itself. */
int wsc_memcpy_h2d_async(wsc_ctx *ctx, void *dst_dev, const void *src_pinned_host, size_t bytes);
int wsc_memcpy_d2h_async(wsc_ctx *ctx, void *dst_pinned_host, const void *src_dev, size_t bytes);

/* timing on the ctx stream with HIP events (bench.py's roofline leg):
 * wsc_timer_begin/_end bracket a region; _end synchronises and returns ms. */
int wsc_timer_begin(wsc_ctx *ctx);
int wsc_timer_end(wsc_ctx *ctx, float *ms_out);

/* Per-kernel-class timing with HIP events on the ctx stream (bench.py's roofline object): between
 * _begin and _end every kernel launch of the ctx is bracketed by an event pair; _end synchronises and
 * returns, per class, the number of launches, their summed duration and their summed algorithmic
 * work (FLOPs for the conv classes, bytes otherwise).  Arrays hold max_classes entries. */
int wsc_profile_begin(wsc_ctx *ctx);
int wsc_profile_end(wsc_ctx *ctx, int max_classes, int32_t *calls_out, float *total_ms_out, double *work_out,
                    int *n_classes_out);
const char *wsc_profile_class_name(int cls);

/* ---- CNN + CAM head --------------------------------------------------- */

/* Build a network from a state_dict.  Replaces model construction +
 * load_state_dict(strict=True) + .eval() + .cuda()
 * (03b_irn/step/make_cam.py:96-100, 33).  Inference BatchNorm
 * (net/resnet50.py:11-14, eps from "<bn>.eps" if given else 1e-5) is folded
 * into per-channel scale/shift applied in the conv epilogue.
 * Missing keys -> WSC_ERR_MISSING_KEY, wrong shapes -> WSC_ERR_SHAPE (the WSC_ARCH_DEEPLAB_* nets: WSC_ERR_SHAPE for both,
 * see wsc_net_forward_seg).
 *
 * Optional key `pool_spec` (WSC_ARCH_VGG16_CAM, WSC_ARCH_M7_CAM), float32 [3][3]: row i = (window, stride, same) of the i-th
 * MaxPooling2D in the order the pools occur -- the three 'M' entries of the VGG16 table; for M7 the two of the stack, then
 * layer3_p2 of the classifier branch.  It carries what a Keras-side session's architecture file says (02_cues/demo.py:104-124,
 * 03c_hsn/utilities.py build_model: model_from_json) where the torch port has MaxPool2d(2, 2) (common_cnn.py:131-132): each pool
 * then follows the rule of wsc_pool_tf_nhwc, wsc_net_cam_size* the sizes it gives (41 at 321 for 3 x 3 / 2 SAME pools), and the
 * M7 classifier branch takes the global maximum of the POOLED map (a VALID pool can leave the last row / column out).  Without
 * the key: the fixed architectures.  Another row count or shape -> WSC_ERR_SHAPE; a non-integral value, a window outside
 * {2, 3}, a stride outside {1, 2} or above the window, same outside {0, 1} -> WSC_ERR_INVALID naming the row; the key on any
 * other arch -> WSC_ERR_INVALID (the IRN flavours keep the torch port's geometry). */
int wsc_net_create(wsc_ctx *ctx, int arch, const wsc_tensor_desc *weights, int n_weights,
                   int num_classes, int precision, wsc_net **out);
void wsc_net_destroy(wsc_net *net);
/* spatial size of the CAM for an S x S input (21 for resnet50 @321, 40 vgg16 @321, 56 m7 @224) */
int wsc_net_cam_size(const wsc_net *net, int S, int *h_out);
/* channels of the last conv feature map (2048 / 1024 / 256) */
int wsc_net_feat_channels(const wsc_net *net, int *f_out);

/* CAM.forward for a batch of B images (resnet50_cam.py:55-70, vgg16_cam.py:24-50):
 *   x_dev   float32 [B][2][3][S][S]  -- per image: original and h-flipped sample,
 *           exactly the "img" tensor of VOC12ClassificationDatasetMSF
 *           (voc12/dataloader.py:240)
 *   cam_dev float32 [B][C][h][w]     -- relu(conv1x1(feat)) of sample 0 plus the
 *           w-flipped map of sample 1
 *   score_dev float32 [B][C] or NULL -- sigmoid(Linear(GAP(feat of sample 0)))
 *           (vgg16_cam.py:34-36); NULL for resnet50 which has no classifier branch
 * Asynchronous on the ctx stream. */
int wsc_net_forward_cam(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int S,
                        float *cam_dev, float *score_dev);
/* The same for NON-SQUARE network inputs x_dev float32 [B][2][3][H][W] -- the reference's resnet50 configuration
 * outsize = None (03b_irn/func_sample.py:143-148): every image goes through the network at its own size, so a device batch
 * holds images of one (H, W).  cam_dev float32 [B][C][h][w] with (h, w) from wsc_net_cam_size_hw. */
int wsc_net_cam_size_hw(const wsc_net *net, int H, int W, int *h_out, int *w_out);
int wsc_net_forward_cam_hw(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float *cam_dev,
                           float *score_dev);

/* Last-conv feature map for Grad-CAM style heads (02_cues/utilities.py:129-132,
 * K.function([input],[conv_output])): feat_dev float32 [N][h][w][F] (NHWC as Keras). */
int wsc_net_forward_features(wsc_ctx *ctx, const wsc_net *net, const float *x_dev /*[N][3][S][S]*/,
                             int N, int S, float *feat_dev);

/* IRNet EdgeDisplacement.forward (03b_irn/net/resnet50_irn.py:210-232, vgg16_irn.py:301-321) for B images,
 * net created with WSC_ARCH_*_IRN from the EdgeDisplacement state dict (backbone keys as for the CAM nets,
 * `fc_edge<k>.0.weight`, `fc_edge<k>.1.{weight,bias}` (GroupNorm), `fc_edge6.{weight,bias}`, `fc_dp<k>...`,
 * `fc_dp7.3.weight`, `mean_shift.running_mean`):
 *   x_dev    float32 [B][2][3][S][S] -- [orig, h-flip] pairs already zero-padded on the right / bottom to the
 *            crop size S (F.pad(x, [0, S - w, 0, S - h]), step/make_sem_seg_labels.py:46 feeds pack['img'][0])
 *   edge_dev float32 [B][feat_h][feat_w] = sigmoid(edge[0]/2 + edge[1].flip(-1)/2), cropped to the feature size
 *            ((h-1)/stride+1, (w-1)/stride+1) of the un-padded image
 *   dp_dev   float32 [B][2][feat_h][feat_w] = displacement field of sample 0 (minus MeanShift.running_mean) */
int wsc_net_forward_edge(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int S, int feat_h, int feat_w,
                         float *edge_dev, float *dp_dev);
/* Net.forward in training mode (resnet50_irn.py:110-133, as AffinityDisplacementLoss.forward calls it, :200) for N plain samples
 * x_dev float32 [N][3][S][S]: no flip pairing, no crop, no mean shift (MeanShift is the identity while training, :105-107) and
 * no sigmoid.  edge_dev float32 [N][He][We] = edge_out, dp_dev float32 [N][2][Hd][Wd] = dp_out, the sizes from
 * wsc_net_edge_size (edge_hw = {He, We}, dp_hw = {Hd, Wd}; equal except for the M7 net, whose edge map is at twice the
 * resolution).  It runs the body of wsc_net_forward_edge: that call's outputs are wsc_irn_edge_finish of these. */
int wsc_net_edge_size(const wsc_net *net, int S, int *edge_hw, int *dp_hw);
int wsc_net_forward_edge_raw(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, float *edge_dev, float *dp_dev);

/* misc.indexing.propagate_to_edge(x, edge, radius, beta, exp_times) -- the IRNet random walk called by
 * 03b_irn/step/make_sem_seg_labels.py:59,76,93 (the `misc` package is missing from the reference tree; the
 * algorithm is upstream IRNet's misc/indexing.py, its affinity step is in-tree as to_affinity,
 * net/vgg16_irn.py:247-261):  rw = (x * (1 - edge)) @ T^(n_steps), T = column-normalised affinity^beta.
 *   x_dev float32 [K][h][w], edge_dev float32 [h][w] (device); rw_dev float32 [K][h][w]
 *   dirs_host int32 [D][2] search directions (dy, dx) of PathIndex (dy > 0, or dy == 0 and dx > 0),
 *   path_start_host int32 [D+1], path_yx_host int32 [path_start[D]][2]: the pixels (relative to the source)
 *   of the straight path of every direction, end points included
 *   n_steps = 2^exp_times applications of T (the reference squares the dense matrix exp_times times) */
int wsc_rw_propagate(wsc_ctx *ctx, const float *x_dev, const float *edge_dev, int K, int h, int w,
                     const int32_t *dirs_host, const int32_t *path_start_host, const int32_t *path_yx_host, int D,
                     float beta, int n_steps, float *rw_dev);
/* The same for n_img images of different sizes in one pass (every stencil step is one launch over all of them --
 * a single 94 x 125 image is launch-bound at ~15 us per step): image b has K_host[b] maps on an h_host[b] x
 * w_host[b] grid; x_dev / rw_dev hold the images' [K][h][w] blocks back to back, edge_dev their [h][w] maps. */
int wsc_rw_propagate_batch(wsc_ctx *ctx, int n_img, const int32_t *K_host, const int32_t *h_host,
                           const int32_t *w_host, const float *x_dev, const float *edge_dev,
                           const int32_t *dirs_host, const int32_t *path_start_host, const int32_t *path_yx_host,
                           int D, float beta, int n_steps, float *rw_dev);

/* Grad-CAM for a plain batch of N samples (02_cues/utilities.py:128-133, 03c_hsn/utilities.py:258-263):
 *   cams[n][y][x][c] = [relu]( sum_f feat[n][y][x][f] * alpha[f][c] )      ('ijkl,lm->ijkm')
 * with alpha the `gradcam_weights` tensor given to wsc_net_create (vgg16 / m7).  One CNN pass
 * yields both the maps and, if score_dev != NULL, sigmoid classifier scores [N][C] -- the
 * reference runs the network twice (model.predict + K.function).
 *   x_dev float32 [N][3][S][S];  cams_dev float32 [N][h][w][C] (NHWC as numpy's einsum result). */
int wsc_net_forward_gradcam(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, int relu,
                            float *cams_dev, float *score_dev);

/* One nn.Conv2d (+ per-channel scale/shift, residual add, ReLU) through the production
 * implicit-GEMM kernel with NCHW float32 tensors on the device -- the unit the per-layer
 * numerics tests drive (conv shape classes of SURVEY.md section 8 a4/a6).  w_host is OIHW.
 * Cin must be <= 4 (stem-style, small-Cin path) or a multiple of 64; Cout a multiple of 8.
 * precision may be OR-ed with WSC_CONV_GENERIC: the layer then runs on the kernel's generic variants instead of the
 * specialised ones the host picks for common layers (same arithmetic; a test holds the two to identical bits). */
#define WSC_CONV_GENERIC 0x100
int wsc_conv2d_nchw(wsc_ctx *ctx, const float *x_dev, int N, int Cin, int H, int W, const float *w_host,
                    int Cout, int kh, int kw, int stride, int pad, const float *scale_host,
                    const float *shift_host, const float *residual_dev, int relu, int precision,
                    float *y_dev);
/* The same with a dilation `dil` >= 1, one rate for both axes (tf.nn.atrous_conv2d's `rate`, DSRG.py:222,268): tap (r, s) of output
 * pixel (ho, wo) reads input (ho * stride - pad + r * dil, wo * stride - pad + s * dil), a tap outside the image contributes
 * zero; the output is (H + 2 pad - ((kh - 1) dil + 1)) / stride + 1 rows.  TF's padding="SAME" for a 3x3 kernel is pad = dil,
 * stride = 1.  dil > 1 needs Cin in multiples of 64 (the generic form) and takes the kernel's per-tap gather, whatever the
 * precision; dil = 1 IS wsc_conv2d_nchw (one implementation, identical bits). */
int wsc_conv2d_nchw_dil(wsc_ctx *ctx, const float *x_dev, int N, int Cin, int H, int W, const float *w_host,
                        int Cout, int kh, int kw, int stride, int pad, int dil, const float *scale_host,
                        const float *shift_host, const float *residual_dev, int relu, int precision,
                        float *y_dev);

/* ---- SEC / DSRG segmentation network (03a_sec-dsrg) ----------------------- */

/* The DeepLab-VGG16 forward pass of SEC / DSRG at drop_prob = 0 (every non-training phase, and the training step of the
 * reference's `debug` graph: the losses and their gradient into fc8 are wsc_seg_loss, the backward pass wsc_net_backward_seg, the
 * SGD-momentum update and the write-back of the weights wsc_seg_sgd_* / wsc_net_seg_load_params below; the `train` phase's
 * dropout behind fc6 / fc7 is wsc_net_forward_seg_train / wsc_net_backward_seg_drop, with the project's own keep-masks).  A net created with WSC_ARCH_DEEPLAB_LFOV / _ASPP takes its weights under the reference's
 * layer names (get_weights_and_bias, DSRG.py:379-425): `conv1_1` ... `conv5_3`, and `fc6`, `fc7`, `fc8` (LFOV) or `fc6_1` ...
 * `fc8_4` (ASPP); each as `<layer>.w` in TensorFlow's HWIO order [kh][kw][Cin][Cout] and `<layer>.b` [Cout].  Channel widths
 * are read from the tensors (multiples of 64; fc8 has num_classes outputs).  A missing or mis-shaped tensor is WSC_ERR_SHAPE
 * and the error text names the layer.  Layers (build_block / build_fc): 3x3 conv + bias + ReLU with padding SAME, conv5_* at
 * rate 2, fc6 at its branch's rate; 3x3 max pools with TF's SAME padding (pad_before = floor(pad_total / 2): 0 / 1 on an even
 * size at stride 2; padding never wins the maximum) at stride 2 (pool1-3) and 1 (pool4, pool5); pool5a, a 3x3 stride-1 average
 * over the in-image taps; dropout is the identity in every entry but wsc_net_forward_seg_train.
 *
 * wsc_net_seg_size_hw: the fc8 map size for an H x W input (41 x 41 at 321 x 321). */
int wsc_net_seg_size_hw(const wsc_net *net, int H, int W, int *h_out, int *w_out);
/* x_dev    float32 [B][H][W][3] NHWC, BGR minus mean: what the reference feeds net["input"] (model.py:337-340)
 * prob_dev float32 [B][h][w][C] NHWC `fc8-softmax` (build_sp_softmax, DSRG.py:297-300 / SEC.py:246-249):
 *          e = exp(x - max), p = e / sum(e) + min_prob, p /= sum(p) over the classes, in fp32 on the fp32 logits --
 *          the layout wsc_dsrg_seed_grow and wsc_seg_unary_nhwc take
 * fc8_dev  NULL, or float32 [B][h][w][C]: the logits (ASPP: fc8_1 + fc8_2 + fc8_3 + fc8_4 in that order, DSRG.py:181)
 * Any H, W >= 1 (non-square and even sizes included).  The IEEE-half modes raise the range flag (WSC_ERR_RANGE at the next
 * synchronising call) as for the other nets; the input itself counts.  Asynchronous on the ctx stream. */
int wsc_net_forward_seg(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob,
                        float *fc8_dev, float *prob_dev);
/* TensorFlow 1.x tf.image.resize_bilinear(align_corners=False) -- the legacy sampler WITHOUT the half-pixel offset of
 * wsc_bilinear_resize -- on NHWC float32: rescale_output (DSRG.py:450 / SEC.py pred), the CRF layer's zoomed image and map
 * (DSRG.py:319-321) and the input resize of image_preprocess (model.py:335).  Per axis scale = in / out (float32),
 * src = dst * scale, i0 = floor(src), i1 = min(i0 + 1, in - 1), t = src - i0; top = tl + (tr - tl) tx, bottom likewise,
 * out = top + (bottom - top) ty.  src_dev [B][h][w][C] -> dst_dev [B][H][W][C]. */
int wsc_resize_bilinear_tf(wsc_ctx *ctx, const float *src_dev, int B, int h, int w, int C, float *dst_dev, int H, int W);
/* The two pieces of that network the per-layer tests drive on their own (float32 NHWC in and out; the values go through the
 * activation planes of `precision` as they do inside the net):
 * wsc_pool_same_nhwc: the 3x3 TF-SAME pool of build_block (DSRG.py:229-246): avg = 0 max at stride 1 / 2, avg = 1 the average
 *   over the in-image taps at stride 1; y_dev [N][ceil(H / stride)][ceil(W / stride)][C], C a multiple of 8.
 * wsc_fc8_softmax: fc8-softmax of the sum of n_in (1 .. 4) float32 [M][C] logit arrays (device pointers in a host array);
 *   sum_dev NULL or [M][C] receives the summed logits. */
int wsc_pool_same_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int avg, int stride, int precision,
                       float *y_dev);
/* TensorFlow / Keras MaxPooling2D(pool_size = k, strides = stride, padding = 'same' | 'valid') on float32 NHWC, through the
 * activation planes of `precision` -- the pool of a `pool_spec` row (wsc_net_create), i.e. of the Keras-side CNNs the drivers
 * of 02_cues/demo.py:104-124 and 03c_hsn/demo.py load from <sess_id>.json.  k 2 or 3, stride 1 or 2 (<= k), same 0 or 1, max
 * only.  Per axis, TensorFlow's rule:
 *   SAME   out = ceil(in / stride), pad_total = max((out - 1) stride + k - in, 0), pad_before = floor(pad_total / 2)
 *   VALID  out = floor((in - k) / stride) + 1, no padding; in < k is WSC_ERR_INVALID
 * Padding never wins the maximum (-inf, not 0).  The two-plane precisions take the maximum of hi + lo; a maximum is one of
 * its inputs, so the result is exact on values the planes hold.  y_dev [N][out_h][out_w][C], C a multiple of 8. */
int wsc_pool_tf_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int k, int stride, int same, int precision,
                     float *y_dev);
/* The small kernels between the convolutions of the torch-side nets, one layer each, for the per-layer tests (float32 in and
 * out; in the entries with a `precision` the values go through the activation planes of that precision as inside the net; the
 * production launchers run unchanged; a bad argument is WSC_ERR_INVALID before anything is launched):
 * wsc_group_norm_nhwc: one IRNet head after its 1 x 1 convolution -- nn.GroupNorm(G, C) (biased variance, eps inside the
 *   square root) of x_dev [N][H][W][C] with gamma_host / beta_host [C], bilinear upsampling by `up` (1, 2 or 4,
 *   align_corners = False), crop to Hd x Wd (<= H up x W up), ReLU if `relu`, written to channels [coff, coff + C) of y_dev
 *   [N][Hd][Wd][Ctot].  y_dev is READ AND WRITTEN: it is staged into the planes first (the concat buffer as the other heads
 *   left it), so its channels outside the slice come back as they went in, rounded to the precision.  WSC_PREC_F32 needs C,
 *   Ctot and coff to be multiples of 4.
 * wsc_maxpool_nhwc: nn.MaxPool2d(k, stride, pad) on NHWC, out = floor((in + 2 pad - k) / stride) + 1 per axis, 2 pad <= k (so
 *   that every window has a tap; padding never wins the maximum), C a multiple of 8.
 * wsc_gap_linear_sigmoid: the classifier branch, score_dev [B][C] = sigmoid(bias + W . pool(feat[sample_stride b])) with
 *   feat_dev [B sample_stride][|hw|][F], the pool the mean over the |hw| positions, or their maximum when hw < 0 (the M7 net);
 *   w_host [C][F], bias_host [C] or NULL; sample_stride 1 or 2 (2: sample 0 of every [image, flipped image] pair).
 * wsc_cam_flip_add: cam_dev [B][C][h][w] = relu(head[2b]) + relu(head[2b + 1]) flipped along w, head_dev [2B][h][w][Cs] NHWC of
 *   which the first C channels are read.
 * wsc_irn_edge_finish: the end of EdgeDisplacement.forward: edge_dev [B][fh][fw] = sigmoid(e[2b] / 2 + flip(e[2b + 1]) / 2) with
 *   e_dev [2B][He][We] cropped to fh x fw BEFORE the flip, dp_dev [B][2][fh][fw] = d[2b] - (ms0, ms1) with d_dev [2B][Hd][Wd][2]. */
int wsc_group_norm_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, const float *gamma_host, const float *beta_host,
                        int G, float eps, int up, int relu, int Hd, int Wd, int Ctot, int coff, int precision, float *y_dev);
int wsc_maxpool_nhwc(wsc_ctx *ctx, const float *x_dev, int N, int H, int W, int C, int k, int stride, int pad, int precision,
                     float *y_dev);
int wsc_gap_linear_sigmoid(wsc_ctx *ctx, const float *feat_dev, int B, int hw, int F, const float *w_host, const float *bias_host, int C,
                           int sample_stride, int precision, float *score_dev);
int wsc_cam_flip_add(wsc_ctx *ctx, const float *head_dev, int B, int h, int w, int C, int Cs, float *cam_dev);
int wsc_irn_edge_finish(wsc_ctx *ctx, const float *e_dev, int He, int We, const float *d_dev, int Hd, int Wd, int B, int fh, int fw,
                        float ms0, float ms1, float *edge_dev, float *dp_dev);
int wsc_fc8_softmax(wsc_ctx *ctx, const float *const *fc8_dev, int n_in, long long M, int C, float min_prob, float *sum_dev,
                    float *prob_dev);

/* ---- backward pass of the SEC / DSRG network: compute_gradients at drop_prob = 0 ------------------------------------------
 * The reference's statement after getloss() is opt.compute_gradients(loss["total"]) (model.py:382-387).  wsc_seg_loss hands out
 * d loss / d fc8; wsc_net_backward_seg carries it to the gradient of every weight and bias of the net, in exact fp32 whatever the
 * net's forward precision.  The definition: the chain rule EVALUATED AT THE TAPE, the fp32 values every op read in the forward
 * pass (hi + lo of a two-plane precision, exact in fp32).  A ReLU passes dy where its kept output is > 0, else +0.0; a max pool
 * sends a window's dy to the window's first maximum in row-major window order (padding is never a candidate); pool5a sends
 * dy / (in-image tap count) to every in-image tap; every ASPP branch receives dfc8 and their gradients into pool5a's output are
 * summed in the order _1 ... _4; no gradient is formed for the network input.  The weight-decay term, the learning-rate
 * multipliers and the optimiser follow below (wsc_seg_sgd_*); dropout: wsc_net_backward_seg_drop below.
 *
 * The tape: wsc_net_seg_tape_plan lists the kept tensors for a B x H x W input -- "input", every op of the trunk ("conv1_1", ...,
 * "pool:0", ..., "pool5a"), every branch's "fc6[_k]" and "fc7[_k]" -- each float32 NHWC [B][Ho][Wo][C] at `offset` floats of one
 * buffer of *tape_elems_out floats; max_entries = 0 for the count.  wsc_net_forward_seg_tape is wsc_net_forward_seg (the same
 * launches, the same bits in fc8_dev / prob_dev) with those tensors copied to the caller's buffer between the launches.  The
 * caller owns the tape; nothing is kept between the forward and the backward pass. */
typedef struct wsc_tape_entry {
    char name[32];
    int32_t Ho, Wo, C;
    int64_t offset; /* floats */
} wsc_tape_entry;
int wsc_net_seg_tape_plan(wsc_ctx *ctx, const wsc_net *net, int B, int H, int W, wsc_tape_entry *entries_out, int max_entries,
                          int *n_out, long long *tape_elems_out);
int wsc_net_forward_seg_tape(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob,
                             float *tape_dev, long long tape_elems, float *fc8_dev, float *prob_dev);
/* ---- dropout: the `train` phase of SEC / DSRG (drop_prob = 0.5, SEC.py:81 / DSRG.py:128) -------------------------------------
 * The sites are drop6 / drop7 behind fc6 / fc7 (SEC.py:123,225-227), drop6_k / drop7_k in each ASPP branch (DSRG.py:174-177,276-278).
 * PARITY WITH TENSORFLOW'S RANDOM STREAM IS UNPINNED: TensorFlow's generator is not reproduced.  The project defines its own
 * counter-based contract, under which a keep-mask depends on (seed, step, site, element index) alone -- never on the launch
 * geometry, the precision, the stream or how a batch is split:
 *   generator  Philox4x32-10: multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85, key = (seed low 32 bits,
 *              seed high 32 bits)
 *   counter    of element i, the linear NHWC index in the [B][h][w][Cout] output of fc6 / fc7: (low 32 bits of i >> 2, high 32 bits
 *              of i >> 2, step, site); element i takes output word i & 3.  step < 2^32, else WSC_ERR_INVALID
 *   site       branch k (0-based; SEC has one) uses 2 k for drop6 and 2 k + 1 for drop7: DSRG's sites 0 .. 7 are independent
 *   keep rule  u = float(word >> 8) 2^-24 (exact); keep iff u >= drop_prob in fp32 -- TF 1.13's random_uniform >= rate.
 *              0 <= drop_prob < 1 (NaN: WSC_ERR_INVALID); drop_prob = 0 keeps everything
 *   value      d = y scale on kept elements, +0.0 on dropped ones; scale = 1.0f / (1.0f - drop_prob), every operation in fp32; the
 *              product is ONE fp32 rounding of the exact value hi + lo of the activation, stored by the split the conv epilogue
 *              uses for the net's precision.  At 0.5 the scale is 2 and everything is exact.  An IEEE half that reaches the
 *              ceiling (a doubled value >= 65504) raises the range flag as a conv epilogue does
 *   tape       keeps its meaning, "the value the next op read": the fc6* / fc7* entries hold the dropped, scaled activations
 *   backward   needs no mask buffer: scale >= 1, so a tape value is > 0 exactly where the unit was kept AND its ReLU output was
 *              positive; fc6 / fc7 form dz = dy scale (one fp32 rounding) there and +0.0 elsewhere, and the bias and weight
 *              gradients follow from that dz.  Nothing but the tape is stored between the passes.
 *
 * wsc_seg_dropout_f32: the kernel on plain fp32, for the tests: y_dev[j] = the dropout of x_dev[j] (y_dev may be x_dev) where
 *   x_dev[0] is element `first` of the logical tensor (so that a small buffer reaches the counter's high word); keep_dev NULL or
 *   `elems` bytes that receive the keep decisions (1 / 0).  Any alignment (16-byte accesses where first is a multiple of 4 and the
 *   buffers allow, else the scalar form: the same words).  Asynchronous on the ctx stream.
 * wsc_net_forward_seg_train: wsc_net_forward_seg_tape with the dropout sites active; in place of the tape copy behind fc6 / fc7
 *   one kernel drops and scales the activation in place and writes the tape entry in the same pass.  At drop_prob = 0 it launches
 *   what wsc_net_forward_seg_tape launches and gives the same bits.
 * wsc_net_backward_seg_drop: wsc_net_backward_seg (below) with scale = 1 / (1 - drop_prob) at the fc6 / fc7 mask step, on a tape
 *   of wsc_net_forward_seg_train at that drop_prob; the same launches.
 * Every argument error is WSC_ERR_INVALID before any launch. */
int wsc_seg_dropout_f32(wsc_ctx *ctx, const float *x_dev, long long elems, long long first, float drop_prob, unsigned long long seed,
                        long long step, int site, float *y_dev, unsigned char *keep_dev);
int wsc_net_forward_seg_train(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float min_prob, float drop_prob,
                              unsigned long long seed, long long step, float *tape_dev, long long tape_elems, float *fc8_dev,
                              float *prob_dev);
/* wsc_seg_grad: what the backward pass of one net keeps -- the rotated, channel-transposed fp32 kernels of the data-gradient
 * convolutions (packed once) and the backward workspace (two gradient activations, the masked dz, the split-K slabs; grown on
 * demand).  `weights`: the list wsc_net_create took; a tensor that is not the net's is WSC_ERR_SHAPE naming the layer.  The net
 * must outlive the object.  wsc_seg_grad_layout: per layer its name, kernel, channels and where dW ([kh][kw][Cin][Cout], TF's
 * HWIO: the layout the weights came in) and db ([Cout]) lie in the gradient buffer of *grad_elems_out floats. */
typedef struct wsc_seg_grad wsc_seg_grad;
typedef struct wsc_grad_entry {
    char name[32];
    int32_t kh, kw, Cin, Cout;
    int64_t w_off, b_off; /* floats */
} wsc_grad_entry;
int wsc_seg_grad_create(wsc_ctx *ctx, const wsc_net *net, const wsc_tensor_desc *weights, int n_weights, wsc_seg_grad **out);
void wsc_seg_grad_destroy(wsc_seg_grad *g);
int wsc_seg_grad_layout(const wsc_seg_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *grad_elems_out);
/* dfc8_dev float32 [B][h][w][C] -> every element of grad_dev (nothing accumulates into the caller's buffer).  ctx: the context
 * the wsc_seg_grad was created on (its workspace belongs to that stream; another one is WSC_ERR_INVALID).  Asynchronous on the
 * ctx stream (the first call at a larger size allocates the workspace).  A tape or gradient size other than the plan's / the
 * layout's is WSC_ERR_INVALID before any launch.  Two calls give the same bits: the split-K slices of a weight gradient are
 * summed in slice order, no floating-point atomic anywhere. */
int wsc_net_backward_seg(wsc_ctx *ctx, wsc_seg_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                         const float *dfc8_dev, float *grad_dev, long long grad_elems);
int wsc_net_backward_seg_drop(wsc_ctx *ctx, wsc_seg_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                              const float *dfc8_dev, float *grad_dev, long long grad_elems, float drop_prob);
/* The layers of that pass one by one, for the per-op tests (float32 NHWC in and out, the launchers of the pass unchanged):
 * wsc_conv2d_wgrad_nhwc: dw_dev [k][k][Cin][Cout] and db_dev [Cout] of a stride-1 SAME convolution (k 1 or 3, pad = dil (k - 1) / 2)
 *   from its input x_dev [N][H][W][Cin] and the gradient dy_dev [N][H][W][Cout] of its (pre-activation) output: fp32 operands on
 *   v_mfma_f32_32x32x2_f32, K = the pixels.  Cin 3 or a multiple of 64; Cout 2 .. 32 (Cin a multiple of 64) or a multiple of 64.
 *   splits = 0: the launcher's choice of K slices, > 0: that many (at most one per K-step of 32 pixels).  A tap outside the image for every pixel is exactly 0.0.
 * wsc_conv2d_dgrad_nhwc: dx_dev [N][H][W][Cin] from dy_dev and the layer's weights w_host [k][k][Cin][Cout]; Cin a multiple of 64.
 * wsc_relu_bias_grad: dz_dev [M][C] = dy [y > 0] (y_dev NULL: dz = dy), db_dev [C] = the column sums of dz.
 * wsc_relu_bias_grad_scaled: the same with dz = dy scale [y > 0], the product one fp32 rounding (the mask step behind a dropout
 *   site; 1 <= scale < inf, 1.0f gives wsc_relu_bias_grad's bits; y_dev NULL: dz = dy, no scale).
 * wsc_pool_same_grad_nhwc: the gradient of wsc_pool_same_nhwc at x_dev [N][H][W][C] (C a multiple of 8) for dy_dev of the pool's
 *   output size -> dx_dev [N][H][W][C]. */
int wsc_conv2d_wgrad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int Cin, int Cout, int k, int dil,
                          int splits, float *dw_dev, float *db_dev);
int wsc_conv2d_dgrad_nhwc(wsc_ctx *ctx, const float *dy_dev, const float *w_host, int N, int H, int W, int Cin, int Cout, int k, int dil,
                          float *dx_dev);
int wsc_relu_bias_grad(wsc_ctx *ctx, const float *y_dev, const float *dy_dev, long long M, int C, float *dz_dev, float *db_dev);
int wsc_relu_bias_grad_scaled(wsc_ctx *ctx, const float *y_dev, const float *dy_dev, long long M, int C, float scale, float *dz_dev,
                              float *db_dev);
int wsc_pool_same_grad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int C, int avg, int stride,
                            float *dx_dev);

/* ---- the update half of the training step: Model.optimize() and the update branch of Model.train() ------------------------------
 * (model.py:379-404, 491-504), whatever the drop_prob of the gradient.  Parameters, the momentum slot and the gradient accumulator are each ONE fp32
 * device buffer of grad_elems floats in the layout of wsc_seg_grad_layout (per layer w in HWIO, then b, no gaps): a gradient
 * buffer of wsc_net_backward_seg, a parameter buffer and a slot buffer are element-for-element parallel.  Both calls are
 * asynchronous on the ctx stream; every product, sum and quotient below is rounded to fp32 on its own (no fused multiply-add).
 *
 * wsc_seg_sgd_accumulate: the graph op `accum_gradient_accum` with the gradient of loss["total"] = norm + weight_decay l2:
 *     t = grad + weight_decay param   on the weights of every layer (fc8 included: l2 sums over weights[layer][0]); t = grad on biases
 *     t = mult t                      mult = 1 (weights), 2 (biases), 10 (fc8 weights), 20 (fc8 biases); fc8 = `fc8`, `fc8_1` .. `fc8_4`
 *     accum += t / accum_num
 *   l2_dev: NULL, or one float that receives loss["l2"] = sum over the layers of sum(w^2) / 2, accumulated in double in one fixed
 *   order (per-block partials, then the last block to arrive -- an integer ticket -- adds them in block order) and rounded once:
 *   two calls give the same bits, no floating-point atomic.  The other outputs do not depend on l2_dev.
 * wsc_seg_sgd_apply: `accum_gradient_update` then (clear_accum) `accum_gradient_clean` -- TensorFlow's ApplyMomentum without
 *   Nesterov on the accumulated gradient: mom = mom momentum + accum, param = param - lr mom; clear_accum: accum = +0.0.
 * Both return WSC_ERR_INVALID before any launch when elems is not the layout's grad_elems, ctx is not the context the
 * wsc_seg_grad was created on (its l2 scratch belongs to that stream), or a pointer that must not be NULL is.
 *
 * wsc_net_seg_load_params: rewrites, in place and without a host copy, everything derived from the weights, from the floats of
 * param_dev: (a) of every convolution of the net (the trunk, fc6 / fc7 / fc8 of every branch) the packed weight rows in the
 * kernel's K order -- the IEEE-half modes with the per-output-channel power-of-two scale taken from the channel's largest |w|,
 * the split modes with both parts --, the epilogue scale and the bias; (b) every layer's rotated, channel-transposed fp32
 * data-gradient kernel in the wsc_seg_grad.  Afterwards the device weights of both objects are byte for byte what wsc_net_create
 * and wsc_seg_grad_create make of the same floats.  `g` must be the wsc_seg_grad of `net`, ctx its context.  The call WRITES the
 * net: the net must not be in use on another stream during it, and work of other streams that reads the net must be ordered
 * behind it by the caller (wsc_ctx_wait).  A net that is no WSC_ARCH_DEEPLAB_* net, a foreign ctx or a wrong elems is
 * WSC_ERR_INVALID before any launch.  Asynchronous on the ctx stream. */
int wsc_seg_sgd_accumulate(wsc_ctx *ctx, wsc_seg_grad *g, const float *param_dev, const float *grad_dev, float *accum_dev,
                           long long elems, float weight_decay, int accum_num, float *l2_dev);
int wsc_seg_sgd_apply(wsc_ctx *ctx, wsc_seg_grad *g, float *param_dev, float *accum_dev, float *mom_dev, long long elems, float lr,
                      float momentum, int clear_accum);
int wsc_net_seg_load_params(wsc_ctx *ctx, wsc_net *net, wsc_seg_grad *g, const float *param_dev, long long elems);

/* The per-op view of a forward pass, for the per-op tests (tests/test_gpu_net_trace.py): what the conv stack of a net does for an
 * N x H x W input, one entry per op in execution order plus one for the CAM head where the net has one, and a forward pass that
 * hands out every op's output.  The IRNet heads and the DeepLab fc6 - fc8 branches run behind the stack and are not listed. */
enum { WSC_TRACE_CONV = 0, WSC_TRACE_POOL = 1, WSC_TRACE_GATHER = 2, WSC_TRACE_HEAD = 3 };
enum { WSC_TRACE_INPUT = -1 /* the operand is the network input */, WSC_TRACE_NONE = -2 /* no such operand */ };
typedef struct wsc_trace_op {
    int32_t kind;         /* WSC_TRACE_CONV / _POOL / _GATHER / _HEAD */
    int32_t in, in2, res; /* index of the entry that wrote the operand LAST: the input, the second source of a stage-entry conv
                             (its last input channels, read at pixel (ho stride2, wo stride2)), the residual; or WSC_TRACE_INPUT /
                             WSC_TRACE_NONE.  An op that reads a concatenated tensor names the op that completed it (the gather) */
    int32_t Ho, Wo;       /* output map */
    int32_t C, coff, pitch; /* the op writes channels [coff, coff + C) of a tensor of `pitch` channels (pitch = C, coff = 0: dense) */
    int32_t kh, kw, stride, pad, dil, relu; /* conv, head; stride also of a gather */
    int32_t affine2;      /* conv: a second affine map follows the ReLU (conv -> bias -> ReLU -> BatchNorm of the plain stacks) */
    int32_t stride2;      /* conv with in2: the pixel stride of the second source, else 0 */
    int32_t pool_rule, pool_k, pool_stride, pool_pad, pool_avg; /* pool: rule 0 torch (pool_pad), 1 TF SAME, 2 TF VALID; avg 0 / 1 */
    int32_t fused_next;   /* 1: this run computes the op together with the next entry and never writes its output (the f16x3 ResNet
                             stem with WSC_OPT_STEM_POOL_FUSED); follows the ctx's options at the time of the call */
    char label[100];      /* the state-dict layers the op implements: "resnet50.layer2.0.conv3+downsample", "vgg16.layer3.0",
                             "conv5_2", "resnet50.layer2.0.gather", "pool:2" (the third pool), "head" */
} wsc_trace_op;
/* Writes min(max_ops, *n_ops_out) entries to ops_out; call with max_ops = 0 for the count. */
int wsc_net_trace_plan(wsc_ctx *ctx, const wsc_net *net, int N, int H, int W, wsc_trace_op *ops_out, int max_ops, int *n_ops_out);
/* The forward pass of the stack (and the head, before the flip-add) with the production launches, and between them a copy of
 * every wanted entry to trace_dev + offsets_host[i] as float32 NHWC [N][Ho][Wo][pitch] -- the WHOLE tensor the op wrote into, hi +
 * lo of the two-plane precisions summed (exact in fp32): the value the next op reads.  Of a tensor wider than the op's own range
 * the other channels are what the buffer held (after the gather of a materialised stage entry: the finished concatenation).
 * offsets_host[i] < 0 skips entry i; n_offsets is the plan's count; a `fused_next` entry must be skipped; every entry must lie in
 * the trace_elems floats of trace_dev.  x_dev float32 [N][3][H][W], or [N][H][W][3] for the WSC_ARCH_DEEPLAB_* nets. */
int wsc_net_forward_trace(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int H, int W, const long long *offsets_host,
                          int n_offsets, float *trace_dev, long long trace_elems);

/* ---- CAM tail ---------------------------------------------------------- */

/* make_cam._work tail for a batch (03b_irn/step/make_cam.py:41-42,62-76 with
 * misc.imutils.get_strided_size / get_strided_up_size):
 * for image b with original size (H0,W0)=size_hw[b], valid classes
 * keys[key_off[b] .. key_off[b+1]) :
 *   strided  = bilinear(cam[b], ((H0-1)/4+1, (W0-1)/4+1), align_corners=False)[keys]
 *   high_res = bilinear(cam[b], (((H0-1)/16+1)*16, ...))[keys][:, :H0, :W0]
 *   each channel divided by (its spatial max + 1e-5)
 * Outputs are packed back to back: image b's strided block starts at float
 * offset strided_off[b] (K_b*h4*w4 floats), high_res at highres_off[b]
 * (K_b*H0*W0 floats); the caller computes the offsets (prefix sums).
 * All descriptor arrays are HOST pointers (copied by the call). */
int wsc_cam_postprocess(wsc_ctx *ctx, const float *cam_dev, int B, int C, int h, int w,
                        const int32_t *size_hw_host /*[B][2]*/, const int32_t *keys_host,
                        const int32_t *key_off_host /*[B+1]*/, const int64_t *strided_off_host /*[B]*/,
                        const int64_t *highres_off_host /*[B]*/, float *strided_dev, float *highres_dev);

/* eval_cam for a batch straight from the packed high_res maps of wsc_cam_postprocess
 * (03b_irn/step/eval_cam.py:48-62 and chainercv.evaluations.calc_semantic_segmentation_confusion):
 *   cams = np.pad(high_res, ((1,0),...), constant_values=bg_thres); keys' = np.pad(keys + 1, (1,0))
 *   pred = keys'[np.argmax(cams, axis=0)];  confusion[gt][pred] += 1 where gt != ignore_label
 * gt_dev / pred_dev: uint8, images packed back to back (H0*W0 each, in batch order); pred_dev may be
 * NULL; gt_dev may be NULL (labels only).  confusion_dev int64 [n_class][n_class] is ACCUMULATED into, so
 * one matrix can be carried over a whole dataset (zero it first with wsc_memset). */
int wsc_cam_eval_confusion(wsc_ctx *ctx, const float *highres_dev, int B, const int32_t *size_hw_host,
                           const int32_t *keys_host, const int32_t *key_off_host,
                           const int64_t *highres_off_host, float bg_thres, const uint8_t *gt_dev, int n_class,
                           int ignore_label, uint8_t *pred_dev, int64_t *confusion_dev);

/* Probabilities -> CRF unaries for a [background | class maps] stack:
 *   v_0 = bg_value, v_{c+1} = maps[b][c][p];  U[b][m][p] = -log(clip(v_m / sum_m v_m, 1e-5, 1))
 * i.e. eval_cam.py:49-51 (np.pad(high_res, constant_values=cam_eval_thres)) followed by
 * pydensecrf.utils.unary_from_softmax (03c_hsn/utilities.py:431).
 *   maps_dev float32 [B][C][N]  ->  unary_dev float32 [B][C+1][N] */
int wsc_unary_from_maps(wsc_ctx *ctx, const float *maps_dev, int B, int C, int N, float bg_value,
                        float *unary_dev);

/* The ADP / DeepGlobe branch of eval_cam (03b_irn/step/eval_cam.py:53-63): no background padding, the keys are class ids,
 *   pred = keys[np.argmax(maps, axis=0)];  pred = cv2.resize(pred, outsize, interpolation=cv2.INTER_NEAREST)
 *   confusion[gt][pred] += 1 where gt != ignore_label
 * maps_dev: image b's [K_b][h_b * w_b] block at float offset maps_off[b] (high_res for ADP, the strided cam for DeepGlobe);
 * gt_dev / pred_dev: uint8 at the OUTPUT size (out_h * out_w per image, packed in batch order; 1088 x 1088 / 2448 x 2448 in
 * the reference).  The nearest-neighbour source index follows cv2: min(floor(x * (1. / (out / src))), src - 1) in double.
 * confusion_dev int64 [n_class][n_class] is accumulated into, as in wsc_cam_eval_confusion. */
int wsc_cam_eval_confusion_nn(wsc_ctx *ctx, const float *maps_dev, int B, const int32_t *src_hw_host /*[B][2]*/,
                              const int32_t *out_hw_host /*[B][2]*/, const int32_t *keys_host, const int32_t *key_off_host /*[B+1]*/,
                              const int64_t *maps_off_host /*[B]*/, const uint8_t *gt_dev, int n_class, int ignore_label,
                              uint8_t *pred_dev, int64_t *confusion_dev);

/* The evaluation tail of the HistoSegNet drivers (03c_hsn/demo.py:386-408): the CRF's label maps (int32, image b's h_b x w_b
 * map at int32 offset labels_off[b]) are resized to the ground truth's size with cv2's INTER_NEAREST rule (as above) and
 * counted:  confusion[gt][pred] += 1 where gt != ignore_label.  The reference's per-class intersections / unions / ground-
 * truth counts are sums over this matrix when every pixel whose colour matches no class is given the extra ground-truth
 * index n_class - 1 (wsscam.hsn.demo.evaluate_labels).  gt_dev / pred_dev uint8 at the output size, packed in batch order. */
int wsc_label_confusion_nn(wsc_ctx *ctx, const int32_t *labels_dev, int B, const int32_t *src_hw_host /*[B][2]*/,
                           const int32_t *out_hw_host /*[B][2]*/, const int64_t *labels_off_host /*[B]*/, const uint8_t *gt_dev,
                           int n_class, int ignore_label, uint8_t *pred_dev, int64_t *confusion_dev);

/* The tail of make_sem_seg_labels for a batch of images (03b_irn/step/make_sem_seg_labels.py:74-79 voc12, :91-96 ADP,
 * :113-118 DeepGlobe), straight from the random-walk maps wsc_rw_propagate_batch left in HBM:
 *   rw_up = F.interpolate(rw, size=up_hw, mode='bilinear', align_corners=False)[..., 0, :H0, :W0]
 *   rw_up = rw_up / torch.max(rw_up)                      (one maximum over all of the image's maps and pixels)
 *   has_bg: rw_up = F.pad(rw_up, (0,0,0,0,1,0), value=bg_thres)          (voc12; keys then hold K + 1 entries)
 *   label = keys[torch.argmax(rw_up, dim=0)]              (first maximum; an all-zero image gives NaN maps: the first of them)
 * rw_dev: image b's [K_b][h_b * w_b] maps at float offset rw_off[b]; khw = (K, h, w); label_dev uint8, H0 * W0 per image,
 * packed in batch order.  Keys must fit a uint8 label. */
int wsc_sem_seg_finish(wsc_ctx *ctx, const float *rw_dev, int B, const int64_t *rw_off_host /*[B]*/, const int32_t *khw_host /*[B][3]*/,
                       const int32_t *up_hw_host /*[B][2]*/, const int32_t *out_hw_host /*[B][2]*/, const int32_t *keys_host,
                       const int32_t *key_off_host /*[B+1]*/, int has_bg, float bg_thres, uint8_t *label_dev);

/* The should_saveimg debug images of every stage for a ragged batch, in one launch: the colour-coded segmentation and its
 * overlay on the input image (03c_hsn/demo.py:183-199, :211-232, :395-418; 02_cues/demo.py:433-477, :604-608;
 * 03a_sec-dsrg/model.py:596-612), from label maps that are already on the device:
 *   pred_idx = cv2.resize(labels, out_hw, INTER_NEAREST)      cv2's rule as above: min(floor(x * (1. / (out / src))), src - 1)
 *   pred_segmask = sum_k (pred_idx == k)[..., None] * palette[k];  a label outside [0, n_colours) -- a negative int32, 255 --
 *                                                             takes other_rgb (zeros in 03c / 02_cues, white in 03a's label2rgb)
 *   overlay[p][ch] = blend[e][ch][img[p][ch]]                  e = the pixel's palette entry, n_colours for 'other'
 * Two nearest stages (mid_hw_host given and image b's entry not 0 x 0: src -> mid -> out, 03c_hsn/demo.py:394,411) are composed
 * per output pixel; no mid-size map is written.  Equal sizes pass the label through.
 * The blend is a TABLE the host builds with the reference's own numpy expression (wsscam.render.blend_table: the float64
 * np.uint8((1 - R) * img + R * mask), or 02_cues' float form handed to imsave), uint8 [n_colours + 1][3][256]: the device does
 * no floating-point blending and so matches numpy for every R.
 * labels_dev: uint8 (WSC_RENDER_LABELS_U8) or int32 (WSC_RENDER_LABELS_I32), image b's h_b x w_b map at ELEMENT offset
 * labels_off[b].  colour_dev, and overlay_dev / img_dev when an overlay is wanted (overlay_dev may be NULL; blend_host and
 * img_dev are then not read): uint8 [out_h][out_w][3] per image at BYTE offset out_off[b], the same offsets in all three
 * (packed back to back: 3 * pixels; any offsets will do, 16-byte stores are used between an image's unaligned head and tail).
 * palette_host uint8 [n_colours][3], other_rgb_host uint8 [3].  Asynchronous on the ctx stream; the host arrays are copied
 * during the call.  WSC_ERR_INVALID, naming the argument, before any launch: a NULL among the required pointers; label_type;
 * B outside 1 .. 65535; n_colours outside 1 .. 63; a size < 1 (mid: 0 x 0 or both >= 1) or a pixel count beyond int32; a
 * negative offset. */
#define WSC_RENDER_LABELS_U8 0
#define WSC_RENDER_LABELS_I32 1
int wsc_render_labels(wsc_ctx *ctx, const void *labels_dev, int label_type /* WSC_RENDER_LABELS_* */, int B,
                      const int32_t *src_hw_host /*[B][2]*/, const int32_t *mid_hw_host /*[B][2] or NULL*/,
                      const int32_t *out_hw_host /*[B][2]*/, const int64_t *labels_off_host /*[B]*/,
                      const int64_t *out_off_host /*[B]*/, const uint8_t *palette_host, int n_colours, const uint8_t *other_rgb_host,
                      const uint8_t *img_dev, const uint8_t *blend_host, uint8_t *colour_dev, uint8_t *overlay_dev);

/* wsc_cam_postprocess (all C classes, every image at H0 x W0) followed by wsc_unary_from_maps, fused: the
 * max-normalised high-resolution maps are never written to HBM, only the unaries are (bit-identical to the
 * two-step path).  Replaces, for a whole batch, make_cam.py:64-76 (upsample to the strided-up size, crop,
 * x /= max + 1e-5) + eval_cam.py:49-51 (background channel) + pydensecrf.utils.unary_from_softmax
 * (03c_hsn/utilities.py:431).
 *   cam_dev float32 [B][C][h][w] (wsc_net_forward_cam)  ->  unary_dev float32 [B][C+1][H0*W0] */
int wsc_cam_unary(wsc_ctx *ctx, const float *cam_dev, int B, int C, int h, int w, int H0, int W0, float bg_value,
                  float *unary_dev);
/* The same with the unaries written PIXEL-major, rows padded to Mp = 4 * ceil((C+1)/4) floats (padding = 0): the layout
 * the mean-field loop reads, for wsc_crf_inference_pm (saves the class-major -> pixel-major pass of wsc_crf_inference).
 *   unary_pm_dev float32 [B][H0*W0][Mp] */
int wsc_cam_unary_pm(wsc_ctx *ctx, const float *cam_dev, int B, int C, int h, int w, int H0, int W0, float bg_value,
                     float *unary_pm_dev);

/* Multi-scale inference (args.cam_scales, 03b_irn/step/make_cam.py:62-69: `torch.sum(torch.stack([F.interpolate(o, size) for
 * o in outputs]), 0)` for the strided and the high-resolution maps): every scale of the MSF dataset is resized to the same
 * network input (voc12/dataloader.py:232-240), so the per-scale CAMs have one size and, bilinear interpolation being linear,
 * the sum of the interpolated maps is the interpolation of the summed map (up to fp32 rounding, ~1e-7 relative).  The scales
 * of an image are consecutive "images" of one wsc_net_forward_cam batch; this adds them in scale order:
 *   cam_dev float32 [n_images * n_scales][map_elems]  ->  out_dev float32 [n_images][map_elems]   (out_dev != cam_dev) */
int wsc_cam_sum_scales(wsc_ctx *ctx, const float *cam_dev, int n_images, int n_scales, long long map_elems, float *out_dev);

/* The MSF dataset transform of a batch of DECODED images (03b_irn/voc12/dataloader.py:68-106, 225-246; constants of
 * adp/dataloader.py:64-80, deepglobe/dataloader.py:60-66): float64 bilinear resize to S x S (cv2.resize INTER_LINEAR
 * on the float64 image, skipped when the image already has that size), float32 normalisation
 * (x - mean[c]) / std[c] (pre_div255: (x / 255 - mean[c]) / std[c], norm_mode 'float'), HWC -> CHW, and with
 * pair = 1 the [x, flip(x, -1)] stack make_cam feeds the network; pair = 0 gives the plain batch of
 * 02_cues/utilities.py:146-181.  Bit-identical to the numpy path of wsscam.voc12.dataloader (same float64 expression).
 *   images_dev uint8: image b is the HWC block [H0_b][W0_b][3] at byte offset_host[b];  size_hw_host int32 [B][2];
 *   x_dev float32 [B][2][3][S][S] (pair) or [B][3][S][S]. */
int wsc_msf_input_u8(wsc_ctx *ctx, const uint8_t *images_dev, int B, const int32_t *size_hw_host,
                     const int64_t *offset_host, int S, const float *mean3_host, const float *std3_host,
                     int pre_div255, int pair, float *x_dev);

/* cv2.resize(uint8 HWC image, (OW, OH)) with the default INTER_LINEAR, for a batch of images of different sizes:
 * read_batch of 02_cues/utilities.py:172-176 and 03c_hsn/utilities.py:170-181 keeps the resized batch as uint8, so the network
 * input AND the CRF image are OpenCV's 8-bit result.  OpenCV's 8U path is fixed point (11-bit coefficients, two passes, the
 * vertical pass (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; exact 2 x 2 decimation = rounded box mean);
 * restated from the published algorithm, cv2 itself is absent offline (parity vs cv2 unpinned).
 *   images_dev uint8: image b is the HWC block [H0_b][W0_b][3] at byte offset_host[b];  size_hw_host int32 [B][2];
 *   out_dev uint8 [B][OH][OW][3]. */
int wsc_resize_u8(wsc_ctx *ctx, const uint8_t *images_dev, int B, const int32_t *size_hw_host, const int64_t *offset_host,
                  int OH, int OW, uint8_t *out_dev);

/* PIL's Image.resize for a ragged batch of uint8 images (csrc/irn_batch.hip): imutils.pil_resize(img, size, order) of upstream
 * IRN -- `Image.fromarray(img).resize(size[::-1], Image.BICUBIC | Image.NEAREST)`, what imutils.random_scale / pil_rescale call
 * (voc12/dataloader.py:169, 236, 280, 317 and the ADP / DeepGlobe twins).  order 3: Resample.c's two-pass bicubic with 22-bit
 * integer coefficients and a uint8 intermediate; order 0: ImagingScaleAffine's nearest index (a running sum in double).  The
 * coefficient and index tables are built on the host in PIL's order of operations; the kernels are integer arithmetic.  Equal to
 * PIL 12 on every byte (tests/test_irn_batch_oracle.py pins the numpy restatement the kernels are tested against).
 *   images_dev uint8: image b is the block [H_b][W_b][channels] at byte offset_host[b];  size_hw_host int32 [B][2];
 *   out_dev uint8: result b is the block [OH_b][OW_b][channels] at byte out_offset_host[b];  out_hw_host int32 [B][2];
 *   channels 1 or 3; order 3 or 0 (anything else: WSC_ERR_INVALID); B 1 .. 65535. */
int wsc_pil_resize_u8(wsc_ctx *ctx, const uint8_t *images_dev, int B, const int32_t *size_hw_host, const int64_t *offset_host,
                      const int32_t *out_hw_host, const int64_t *out_offset_host, int channels, int order, uint8_t *out_dev);

/* One IRNet training batch from decoded images and their IR labels (csrc/irn_batch.hip): the sample transform of
 * VOC12AffinityDataset.__getitem__ (voc12/dataloader.py:270-321; adp/dataloader.py:270-321, deepglobe/dataloader.py:257-308), in
 * the reference's order --
 *   1. resize     stage 0: none (the sample must be scaled_h x scaled_w already); stage 1: imutils.random_scale's PIL rescale
 *                 to scaled_h x scaled_w (:280; bicubic on the image, nearest on the label); stage 2: TorchvisionResize to
 *                 scaled_h x scaled_w (:282-284; the float64 bilinear of wsc_msf_input_u8 on the image AND the label, the label
 *                 truncated to uint8 as np.uint8 inside pil_resize does at :317 -- the vgg16 / m7 configuration)
 *   2. normalise  (:286-287) (v - mean[c]) / std[c], one fp32 subtract and one fp32 divide; pre_div255: v / 255 first
 *   3. flip       (:289-290) np.fliplr of the resized image and label where flip = 1
 *   4. crop       (:292-296) an S x S container of 0.0 (image) / 255 (label);
 *                 container[cont_top : cont_top + ch, cont_left : cont_left + cw] = img[img_top : img_top + ch, img_left : img_left + cw]
 *   5. HWC -> CHW (:298), and imutils.pil_rescale(label, 0.25, 0) of the cropped label (:317): s = round-half-even(S / 4)
 *   images_dev uint8: sample b's image [H_b][W_b][3] at byte image_offset_host[b]; labels_dev uint8: its label [H_b][W_b] at byte
 *   label_offset_host[b]; size_hw_host int32 [B][2];
 *   params_host int32 [B][9]: {scaled_h, scaled_w, flip, cont_top, cont_left, img_top, img_left, ch, cw};
 *   x_dev float32 [B][3][S][S]; label_dev uint8 [B][S][S]; reduced_dev uint8 [B][s][s].
 * WSC_ERR_INVALID, naming the sample and before any launch: a window that leaves the resized image or the container, stage 0 on a
 * sample of another size, B outside 1 .. 65535.  The temporary (the horizontal pass's rows) is a cached block of the context. */
int wsc_irn_train_batch(wsc_ctx *ctx, const uint8_t *images_dev, const uint8_t *labels_dev, int B, const int32_t *size_hw_host,
                        const int64_t *image_offset_host, const int64_t *label_offset_host, const int32_t *params_host, int S,
                        const float *mean3_host, const float *std3_host, int pre_div255, int stage, float *x_dev,
                        uint8_t *label_dev, uint8_t *reduced_dev);

/* F.interpolate(mode='bilinear', align_corners=False) on float32 [C][h][w] -> [C][H][W]
 * (make_cam.py:64-69; also resize_stack 02_cues/utilities.py:20-40 up to the
 * cv2/torch border convention). */
int wsc_bilinear_resize(wsc_ctx *ctx, const float *src_dev, int C, int h, int w, float *dst_dev, int H,
                        int W);

/* ---- cam_to_ir_label (03b_irn/step/cam_to_ir_label.py:26-75) ------------------------------- */

/* labels = np.argmax(np.pad(high_res, ((1,0),(0,0),(0,0)), constant_values=thres), axis=0) and the unary energy of
 * imutils.crf_inference_label: pydensecrf.utils.unary_from_labels(labels, n_labels = K + 1, gt_prob, zero_unsure=False).
 *   highres_dev float32 [B][K][N];  unary_dev float32 [B][K+1][N];  labels_dev int32 [B][N] or NULL. */
int wsc_label_unary_from_cam(wsc_ctx *ctx, const float *highres_dev, int B, int K, int N, float thres, float gt_prob,
                             float *unary_dev, int32_t *labels_dev);
/* conf = keys[fg_pred]; with bg_pred_dev (VOC, :54-57): conf[fg_conf == 0] = 255, conf[bg_conf + fg_conf == 0] = 0;
 * without (ADP / DeepGlobe, keys[0] = -1, :38-40 / :71-73): conf[fg_conf == -1] = 255.
 *   fg_pred_dev / bg_pred_dev int32 [B][N] (CRF arg-max);  keys_host int32 [B][M];  conf_dev uint8 [B][N]. */
int wsc_ir_label_combine(wsc_ctx *ctx, const int32_t *fg_pred_dev, const int32_t *bg_pred_dev, const int32_t *keys_host,
                         int B, int M, int N, uint8_t *conf_dev);

/* ---- SEC / DSRG (03a_sec-dsrg): the host py_funcs of the training graph ------------------------ */

/* DSRG seeded region growing (03a_sec-dsrg/DSRG.py:7-62 single_generate_seed_step, batch driver :356-371): per image,
 * e = prob * tag, the candidate class of a pixel by the mask arithmetic of :28-39 (arg-max over the tagged classes, foreground
 * above th_f / background above th_b), and for every tagged class c the connected components of the pixels whose candidate
 * is c; a component that holds a pixel with cue[p][c] == 1 gets cue[p][c] = 1 everywhere except on pixels that are seeded for
 * exactly one other class (those still connect).  Nothing is ever cleared.
 * ASSUMPTION: the reference's labeller lib/CC_labeling_8.py is not in the reference tree; by its name and upstream DSRG the
 * components are 8-CONNECTED, label 0 means "not a candidate of c", and such pixels are never filled.
 *   tags_dev  float32 [B][C]          0/1
 *   cues_dev  float32 [B][H][W][C]    0/1   (NHWC, as the reference's py_func receives it)
 *   probs_dev float32 [B][H][W][C]
 *   out_dev   float32 [B][H][W][C]    may be the same buffer as cues_dev
 * th_f / th_b are arguments (reference constants 0.5 / 0.7).  1 <= C <= 32; H * W <= 8192 (an image's label plane lives in
 * LDS; the reference's maps are 41 x 41, model.py:35): WSC_ERR_INVALID beyond, before any launch. */
int wsc_dsrg_seed_grow(wsc_ctx *ctx, const float *tags_dev, const float *cues_dev, const float *probs_dev,
                       int B, int H, int W, int C, float th_f, float th_b, float *out_dev);

/* The loss head of the training graph and the gradient it sends into fc8 (03a_sec-dsrg/SEC.py:363-465 getloss, get_seed_loss,
 * get_expand_loss, get_constrain_loss; DSRG.py:459-518 getloss, get_balanced_seed_loss, get_constrain_loss).  `crf` and the cues
 * come out of tf.py_func in the reference graph, so they are constants to the gradient: no backward pass through the CRF or the
 * region growing.  The backward pass of the convolution stack is wsc_net_backward_seg, the weight decay term and the optimiser
 * wsc_seg_sgd_*, the `train` phase's dropout wsc_net_forward_seg_train / wsc_net_backward_seg_drop.
 *   prob_dev   float32 [B][H][W][C]  fc8-softmax p (wsc_net_forward_seg), > 0;  n = H W
 *   crf_dev    float32 [B][H][W][C]  the CRF layer's log-probabilities (wsc_seg_crf_logprob);  q = exp(crf)
 *   cues_dev   float32 [B][H][W][C]  0/1 (DSRG: the grown cues of wsc_dsrg_seed_grow)
 *   labels_dev float32 [B][C]        SEC only (NULL for DSRG), class 0 = background;  stat_bc = labels[b][c] > 0 for c >= 1
 * WSC_SEG_LOSS_SEC:
 *   seed      = -(1/B) sum_b [sum cues log p]_b / max([sum cues]_b, 1e-5)
 *   constrain = (1/(B n)) sum q log(q / p)
 *   mean_bc   = sum_i sorted_i w_i / Z over the ascending sort of map (b, c), w = w_fg_host, Z = z_fg for c >= 1 (q_fg = 0.996),
 *               w_bg_host, z_bg for c = 0 (q_bg = 0.999);  max_bc = the map's maximum
 *   loss_1    = -(1/B) sum_b sum_c stat log(mean) / max(sum_c stat, 1e-5)
 *   loss_2    = -(1/B) sum_b sum_c (1 - stat) log(1 - max) / max(sum_c (1 - stat), 1e-5)
 *   loss_3    = -(1/B) sum_b log(mean_b0);   expand = loss_1 + loss_2 + loss_3;   norm = seed + expand + constrain
 *   The weight tables [n] are the reference's constants as TensorFlow sees them: float32(w64) and float32(np.sum(w64)) of
 *   w64 = [q ** i for i in range(n - 1, -1, -1)].  The caller forms them (secdsrg.rank_weights); they are copied during the call.
 * WSC_SEG_LOSS_DSRG (labels, weight tables and sums are not read):
 *   seed_bg   = -(1/B) sum_b [sum cues_0 log p_0]_b / ([sum cues_0]_b + 1e-8);  seed_fg likewise over the channels 1 .. C-1
 *   seed      = seed_bg + seed_fg;   constrain = (1/(B n)) sum q log(q / (p + 1e-8) + 1e-8);   norm = seed + constrain
 * loss_dev double [WSC_SEG_LOSS_N], indexed by the WSC_SEG_LOSS_* slots below; a slot the method lacks is 0.
 * Gradient of norm, both optional (NULL: not computed, the buffer is not touched), float32 [B][H][W][C], every element written:
 *   grad_prob_dev  g_p = d norm / d p.  Seed and constrain terms per element; loss_1 / loss_3 give pixel x of map (b, c)
 *                  -(1/B) coeff_bc (w[rank(x)] / Z) / mean_bc; loss_2 gives +(1/B) coeff_bc / (1 - max_bc) to the maximum.
 *   grad_fc8_dev   g_z = s (g_p - sum_j g_p,j s_j) / (1 + C min_prob) with s = p (1 + C min_prob) - min_prob, the chain rule
 *                  through build_sp_softmax (SEC.py:246-249): d norm / d fc8.  DSRG's fc8 is the sum of fc8_1 .. fc8_4, so the
 *                  same array is the gradient of each of them.
 *   Both may be requested in one call.  They must not overlap each other or any input.
 * TIE RULES: among equal values of a map the lower pixel index gets the lower rank (np.argsort(kind='stable')); the loss values
 * do not depend on it, the placement of the rank weights inside a tied group does.  The share of the maximum is split EQUALLY
 * among the pixels that hold it (TensorFlow's reduce_max gradient).  -0 counts as +0; NaN is out of contract.
 * ARITHMETIC: inputs are float32; every log, exp, product and sum runs in double and each output is rounded once.  Every sum
 * has one fixed order and there are no floating-point atomics: two calls on the same input give the same bits.  TensorFlow
 * evaluates the same graph in float32 with its own summation order: parity with it is UNPINNED.
 * Limits, checked before any launch (WSC_ERR_INVALID, the text names the argument): H * W <= 8192 (a map is sorted in LDS),
 * 2 <= C <= 32, 1 <= B <= 65535, 0 <= min_prob < 1; no NULL among prob_dev, crf_dev, cues_dev, loss_dev and, for SEC,
 * labels_dev and the weight tables.  Asynchronous on the ctx stream. */
#define WSC_SEG_LOSS_SEC 0
#define WSC_SEG_LOSS_DSRG 1
enum {
    WSC_SEG_LOSS_SEED = 0,  /* self.loss["seed"] */
    WSC_SEG_LOSS_CONSTRAIN, /* self.loss["constrain"] */
    WSC_SEG_LOSS_EXPAND,    /* self.loss["expand"] (SEC) */
    WSC_SEG_LOSS_1,         /* SEC self.loss_1 */
    WSC_SEG_LOSS_2,         /* SEC self.loss_2 */
    WSC_SEG_LOSS_3,         /* SEC self.loss_3 */
    WSC_SEG_LOSS_NORM,      /* getloss's return value */
    WSC_SEG_LOSS_SEED_BG,   /* DSRG loss_bg */
    WSC_SEG_LOSS_SEED_FG,   /* DSRG loss_fg */
    WSC_SEG_LOSS_N
};
int wsc_seg_loss(wsc_ctx *ctx, int method /* WSC_SEG_LOSS_SEC | WSC_SEG_LOSS_DSRG */, const float *prob_dev, const float *crf_dev,
                 const float *cues_dev, const float *labels_dev /* [B][C]; SEC only, NULL for DSRG */, int B, int H, int W, int C,
                 float min_prob, const float *w_fg_host, float z_fg, const float *w_bg_host, float z_bg /* [H*W] each; SEC only */,
                 double *loss_dev /* [WSC_SEG_LOSS_N] */, float *grad_prob_dev /* or NULL */, float *grad_fc8_dev /* or NULL */);

/* ---- 03b_irn: the training loss of step/train_irn.py and its gradient into the two head outputs ------------------------------
 * AffinityDisplacementLoss.forward's four loss tensors (net/resnet50_irn.py:162-213 to_affinity, to_pair_displacement,
 * to_displacement_loss, forward), the pair labels of GetAffinityLabelFromIndices (voc12/dataloader.py:115-131) and the
 * reductions of step/train_irn.py:114-125, without any of the per-pair tensors:
 *   edge_dev  float32 [B][h][w]     edge_out BEFORE the sigmoid (wsc_net_forward_edge_raw)
 *   dp_dev    float32 [B][2][h][w]  dp_out
 *   label_dev uint8   [B][h][w]     the reduced IR label (imutils.pil_rescale(label, 0.25, 0), voc12/dataloader.py:317)
 *   dirs_host, path_start_host, path_yx_host, D: the PathIndex tables exactly as wsc_rw_propagate takes them
 *   radius_floor rf = ceil(radius) - 1; valid_below: labels >= it are ignored (21 in all three dataloaders, :122; 255 = ignore)
 * Sources are the pixels (y, x) with y < h - rf and rf <= x < w - rf; pair (s, d) joins s to t = s + dir_d.  Per pair
 *   valid = L(s) < valid_below and L(t) < valid_below;  bg = valid and L(s) == L(t) == 0;  fg = valid and L(s) == L(t) > 0;
 *   neg = valid and L(s) != L(t)
 *   m = the maximum of the edge LOGITS over the path's pixels (the sigmoid is monotonic: the reference's maximum of the
 *       sigmoids is the sigmoid of m);  aff = 1 - sigmoid(m);  pos = -log(aff + 1e-5);  neg = -log(1 + 1e-5 - aff)
 *   pd_c = dp_c(s) - dp_c(t);  fgl = |pd_0 - dy| + |pd_1 - dx| with (dy, dx) = dir_d (disp_target);  bgl = |pd_0| + |pd_1|
 * and over the WHOLE batch, with n_bg, n_fg, n_neg the pair counts:
 *   pos_bg = sum(bg pos) / (n_bg + 1e-5);  pos_fg = sum(fg pos) / (n_fg + 1e-5);  pos = pos_bg / 2 + pos_fg / 2
 *   neg    = sum(neg neg) / (n_neg + 1e-5)
 *   dp_fg  = sum(fg fgl) / (2 n_fg + 1e-5);  dp_bg = sum(bg bgl) / (2 n_bg + 1e-5)
 *   total  = (pos + neg) / 2 + (dp_fg + dp_bg) / 2
 * loss_dev double [WSC_IRN_LOSS_N], the slots below.  Gradients of total, both optional (NULL: not computed, the buffer is not
 * touched), every element written, +0.0 where no pair reaches: grad_edge_dev float32 [B][h][w], grad_dp_dev float32 [B][2][h][w].
 * TIE RULES: the gradient of a path maximum goes to the FIRST pixel that holds it in stored path order (destination first),
 * F.max_pool2d's rule; d|v|/dv at v == 0 is 0, as torch has it.
 * ARITHMETIC: inputs are float32; every sigmoid, log, product and sum runs in double and each output is rounded once; the
 * sigmoid is stable for any finite logit.  Per-pixel pair counts are integers (integer atomics: exact whatever the order);
 * every floating-point sum has one fixed order and there is no floating-point atomic: two calls give the same bits.  The
 * reference evaluates in float32, where 1 - sigmoid loses digits near saturation and count + 1e-5 rounds the 1e-5 away:
 * parity with float32 torch is UNPINNED.
 * Limits, checked before any launch (WSC_ERR_INVALID, the text names the argument): h > rf, w > 2 rf, 0 <= rf <= 16 (a tile and
 * its halo live in LDS), 1 <= B <= 65535, D >= 1, 1 <= valid_below <= 255, every path non-empty, every direction and path
 * offset inside [0, rf] x [-rf, rf]; no NULL among edge_dev, dp_dev, label_dev, loss_dev and the tables; the gradients overlap
 * neither the inputs nor each other.  Asynchronous on the ctx stream. */
enum {
    WSC_IRN_LOSS_POS_BG = 0, /* bg_pos_aff_loss */
    WSC_IRN_LOSS_POS_FG,     /* fg_pos_aff_loss */
    WSC_IRN_LOSS_POS,        /* pos_aff_loss, 'loss1' */
    WSC_IRN_LOSS_NEG,        /* neg_aff_loss, 'loss2' */
    WSC_IRN_LOSS_DP_FG,      /* dp_fg_loss, 'loss3' */
    WSC_IRN_LOSS_DP_BG,      /* dp_bg_loss, 'loss4' */
    WSC_IRN_LOSS_TOTAL,      /* total_loss */
    WSC_IRN_LOSS_N_BG,       /* sum(bg_pos_label) */
    WSC_IRN_LOSS_N_FG,       /* sum(fg_pos_label) */
    WSC_IRN_LOSS_N_NEG,      /* sum(neg_label) */
    WSC_IRN_LOSS_N
};
int wsc_irn_aff_loss(wsc_ctx *ctx, const float *edge_dev, const float *dp_dev, const uint8_t *label_dev, int B, int h, int w,
                     const int32_t *dirs_host, const int32_t *path_start_host, const int32_t *path_yx_host, int D, int radius_floor,
                     int valid_below, double *loss_dev /* [WSC_IRN_LOSS_N] */, float *grad_edge_dev /* or NULL */,
                     float *grad_dp_dev /* or NULL */);

/* ---- 01_train: the loss head of the classifier with the gradient through the head, and the score side of predict() -----------
 * wsc_cls_loss is model.compile(loss='binary_crossentropy', metrics=['binary_accuracy', f1]) (01_train/demo.py:60-61,
 * utilities.py:69-97) on the head global pool -> Dense -> sigmoid, with the gradient of the loss through that head.  The backward
 * pass through the plain stacks and BatchNorm in training mode follow below (wsc_net_backward_cls), then the Nesterov SGD step
 * with the repack of the updated weights (wsc_cls_sgd_step, wsc_net_cls_load_params), then the generators' sample transform
 * (wsc_cls_train_batch).
 *   feat_dev      float32 [B][n][F]  the NHWC map the head reduces, as wsc_net_forward_features writes it; n = h w
 *   pool          WSC_CLS_POOL_MEAN: the mean over the n positions (VGG16);  WSC_CLS_POOL_MAX: their maximum (M7) -- the two
 *                 cases of wsc_gap_linear_sigmoid
 *   w_dev         float32 [C][F]     Dense weights;   bias_dev float32 [C] or NULL
 *   target_dev    float32 [B][C]     targets z, 0/1
 *   sample_w_host float32 [B] or NULL: per-sample weights w_b, NULL = ones; copied during the call
 * With l the logit, p = sigmoid(l), eps = float32(1e-7) (K.epsilon()), hi = float32(1) - eps (a float32 subtraction: 1 - 2^-23)
 * and p_c = clip(p, eps, hi):
 *   l_b  = (1/C) sum_c -(z log p_c + (1 - z) log(1 - p_c))          the per-sample loss (K.mean(K.binary_crossentropy, axis=-1))
 *   L    = sum_b w_b l_b / #{b : w_b != 0}                           Keras' weighted_masked_objective
 *   n_equal = #{z == round(p)};  tp = sum round(z p);  possible = sum round(z);  predicted = sum round(p)
 *   with round half to even, so p = 0.5 rounds to 0.  binary_accuracy = n_equal / (B C); recall = tp / (possible + 1e-7),
 *   precision = tp / (predicted + 1e-7), f1 = 2 precision recall / (precision + recall + 1e-7): the caller forms the ratios.
 * loss_dev double [WSC_CLS_LOSS_N], the slots below (the counts are integers held in doubles); score_dev float32 [B][C] =
 * float32(p), optional.
 * Gradients of L, each optional (NULL: not computed, the buffer is not touched), every element written:
 *   g_l[b][c]     = (w_b / (C #{w != 0})) (p - z) where eps <= p <= hi, else +0.0 (TensorFlow's clip_by_value gradient)
 *                 (a sample of weight 0 has g_l = +0.0 as well: its rows of grad_feat_dev are +0.0 to the bit)
 *   grad_w_dev    float32 [C][F]     sum_b g_l[b][c] pooled[b][f]
 *   grad_bias_dev float32 [C]        sum_b g_l[b][c]
 *   grad_feat_dev float32 [B][n][F]  from g_pooled[b][f] = sum_c g_l[b][c] W[c][f]: mean pool g_pooled / n at every position; max
 *                 pool g_pooled / (positions that hold the maximum) at each of them, +0.0 elsewhere
 * TIE RULES: the share of a maximum is split EQUALLY among the positions that hold it (TensorFlow's reduce_max gradient, the
 * rule of wsc_seg_loss); -0 counts as +0; NaN is out of contract.
 * ARITHMETIC: inputs are float32; every sum, product, sigmoid and log runs in double and each output is rounded once.  p and
 * 1 - p are both formed from exp(-|l|), so the sigmoid and log(1 - p_c) are stable for any finite logit.  Every floating-point sum
 * has one fixed order (the pooled reduction: fixed chunks of positions, combined in chunk order) and there is no floating-point
 * atomic: two calls give the same bits.  Keras evaluates the same graph in float32: parity with it is UNPINNED.  In particular
 * what Keras does with the LIST class_weight of demo.py:80-82,107 is not reproduced: the interface takes per-sample weights only.
 * Limits, checked before any launch (WSC_ERR_INVALID, the text names the argument): 1 <= B <= 1024, 1 <= C <= 64, F a multiple of
 * 4 and <= 4096, 1 <= n <= 65536; a negative or non-finite weight, or no non-zero weight; no NULL among feat_dev, w_dev,
 * target_dev, loss_dev; feat_dev, w_dev, grad_feat_dev and grad_w_dev 16-byte aligned; no output overlaps an input or another
 * output.  Asynchronous on the ctx stream. */
#define WSC_CLS_POOL_MEAN 0
#define WSC_CLS_POOL_MAX 1
enum {
    WSC_CLS_LOSS_TOTAL = 0, /* L, the value Keras reports as `loss` */
    WSC_CLS_LOSS_MEAN,      /* (1/B) sum_b l_b, unweighted */
    WSC_CLS_LOSS_N_EQUAL,   /* #{z == round(p)} */
    WSC_CLS_LOSS_TP,        /* sum round(z p) */
    WSC_CLS_LOSS_POSSIBLE,  /* sum round(z) */
    WSC_CLS_LOSS_PREDICTED, /* sum round(p) */
    WSC_CLS_LOSS_N
};
int wsc_cls_loss(wsc_ctx *ctx, const float *feat_dev, int B, int n, int F, int pool /* WSC_CLS_POOL_MEAN | WSC_CLS_POOL_MAX */,
                 const float *w_dev, const float *bias_dev /* or NULL */, int C, const float *target_dev,
                 const float *sample_w_host /* [B] or NULL */, double *loss_dev /* [WSC_CLS_LOSS_N] */, float *score_dev /* or NULL */,
                 float *grad_feat_dev /* or NULL */, float *grad_w_dev /* or NULL */, float *grad_bias_dev /* or NULL */);

/* get_optimal_thresholds (01_train/utilities.py:99-114): per class the threshold of sklearn's roc_curve(drop_intermediate=True) at
 * the first minimum of |tpr - (1 - fpr)|.  score_dev float32 [N][C], target_dev float32 [N][C] 0/1 (positive: == 1).  Per class:
 *   1. the scores in their distinct values, descending (-0 counts as +0);
 *   2. at the end of each group tps = positives so far, fps = (samples so far) - tps;
 *   3. interior point i is dropped when fps[i-1] - 2 fps[i] + fps[i+1] and tps[i-1] - 2 tps[i] + tps[i+1] are both 0; the first
 *      and the last point always stay;
 *   4. ONLY THEN the point (0, 0) with threshold +inf is put in front.
 *   tpr = tps / P, fpr = fps / Nn (double divisions, P / Nn the positive / negative samples); the threshold is the one at the
 *   FIRST minimum of |tpr - (1 - fpr)|, evaluated in double in exactly that order.
 * A class without a positive or without a negative sample returns +inf and sets WSC_ROC_NO_POSITIVE / WSC_ROC_NO_NEGATIVE in
 * status_dev[c] (sklearn yields NaN rates there and argmin returns 0); a class whose scores are all equal returns +inf too (both
 * points are at distance 1).  thresh_dev float32 [C], status_dev int32 [C]; optional: n_points_dev int32 [C] (the kept points, the
 * one in front included) and, together, fps_dev / tps_dev int32 [C][N + 1] (zeros behind the kept points) -- class_fprs /
 * class_tprs are these over Nn / P.  Every output is an integer or a copy of an input score: exact.
 * Limits, checked before any launch (WSC_ERR_INVALID): 1 <= N <= 16384 (a class is sorted in LDS; beyond 64 KiB the launch limit
 * is raised first and a refusal fails the call), 1 <= C <= 64.  NaN is out of contract.  Asynchronous on the ctx stream. */
#define WSC_ROC_NO_POSITIVE 1
#define WSC_ROC_NO_NEGATIVE 2
int wsc_roc_thresholds(wsc_ctx *ctx, const float *score_dev, const float *target_dev, int N, int C, float *thresh_dev,
                       int32_t *status_dev, int32_t *n_points_dev /* or NULL */, int32_t *fps_dev /* or NULL */,
                       int32_t *tps_dev /* or NULL */);

/* The counts of get_thresholded_metrics_class / _overall (utilities.py:118-165) with pred = score >= thresh_dev[c] (float32
 * comparison; thresh_dev float32 [C] on the device, +inf allowed): counts_dev int64 [C][WSC_CLS_COUNT_N] = TP (target == 1 and
 * pred), FP (target == 0 and pred), TN, FN and #{target == pred}; the caller forms the ratios, per class and from the sums over
 * the classes.  Integer atomics: exact whatever the order.  1 <= N <= 16384, 1 <= C <= 64.  Asynchronous on the ctx stream.
 * wsc_cls_scores_append copies elems floats from src_dev to dst_dev on the stream (the batches of a prediction pass into one
 * [N][C] array); the two must not overlap. */
enum { WSC_CLS_COUNT_TP = 0, WSC_CLS_COUNT_FP, WSC_CLS_COUNT_TN, WSC_CLS_COUNT_FN, WSC_CLS_COUNT_EQUAL, WSC_CLS_COUNT_N };
int wsc_cls_threshold_counts(wsc_ctx *ctx, const float *score_dev, const float *target_dev, int N, int C, const float *thresh_dev,
                             int64_t *counts_dev /* [C][WSC_CLS_COUNT_N] */);
int wsc_cls_scores_append(wsc_ctx *ctx, const float *src_dev, long long elems, float *dst_dev);

/* ---- 01_train: training-mode forward and backward pass of the plain stacks (WSC_ARCH_VGG16_CAM / WSC_ARCH_M7_CAM) ---------------
 * The graph is common_cnn.make_layers' (03b_irn/net/common_cnn.py:128-141): conv(bias) -> ReLU -> BatchNorm(eps = 1e-3) per entry,
 * the max pools between (MaxPool2d(2, 2), or the rows of `pool_spec`).  The `D` dropout entries (VGG16's layer5, M7's classifier
 * branch) are the identity in the two entry points of this block and active in the *_drop entry points of the next one;
 * the data generators, Keras' list class_weight and the writing of .h5 files are not here (the Nesterov SGD
 * step and the repack of updated weights follow this section).  wsc_cls_loss hands out d loss / d feat on the last feature map (and the gradient of the classifier's
 * Linear); wsc_net_backward_cls carries it to every conv and BatchNorm parameter in exact fp32 whatever the forward precision.  The
 * definition is the chain rule EVALUATED AT THE TAPE, as for the other two nets: a ReLU passes dy where its kept output is > 0, a
 * max pool sends a window's dy to the window's first maximum in row-major window order (recomputed from its kept input; padding is
 * never a candidate; overlapping windows add in window order), BatchNorm's backward takes xh = (a - mean) rstd from the taped input
 * and the taped float {mean, rstd}; no gradient is formed for the network input.
 *
 * wsc_batch_norm_train_nhwc: BatchNorm in training mode on a_dev float32 [M][C] (M = N H W), asynchronous on the ctx stream.
 *   Per channel the mean and the POPULATION variance are accumulated in double in one fixed order (per-block partial sums of
 *   a - a[0][c] and its square, the last block to arrive -- an integer ticket -- adds them in block order): no floating-point atomic,
 *   two calls give the same bits.  stats_dev float32 [C][2] = {mean, rstd}, rstd = 1 / sqrt(var + eps) formed in double, each
 *   rounded once.  y_dev float32 [M][C] = fma((a - mean) rstd, gamma, beta) in fp32 from those floats (the difference and the
 *   product one rounding each).  gamma_dev / beta_dev float32 [C] on the device.
 *   run_dev: NULL, or float32 [2][C] (running mean, then running variance), updated in place:
 *     run = keep run + (1 - keep) batch, in double from the unrounded batch value, rounded once; with `unbiased` the batch variance
 *     is multiplied by M / (M - 1) first.  `keep` IS THE WEIGHT OF THE OLD VALUE: Keras' BatchNormalization(momentum = 0.99) is
 *     keep = 0.99, while the torch port's nn.BatchNorm2d(v, eps=0.001, momentum=0.99) (common_cnn.py:138) weighs the NEW value
 *     with its momentum, i.e. keep = 0.01.  KERAS 2.2'S OWN FACTOR ON THE MOVING VARIANCE IS UNPINNED; the contract is torch's /
 *     TensorFlow's fused batch norm: unbiased = 1.
 *   WSC_ERR_INVALID before any launch: a NULL among a_dev, gamma_dev, beta_dev, stats_dev, y_dev; C no multiple of 4 or > 1024;
 *   M < 1 or >= 2^31; M == 1 with `unbiased`; eps < 0 or not finite; keep outside [0, 1] with run_dev given; a_dev / y_dev not
 *   16-byte aligned.
 * wsc_batch_norm_grad_nhwc: its backward pass from a_dev, the taped stats_dev (nothing is recomputed), gamma_dev and the gradient
 *   dy_dev [M][C] of y:  dbeta = sum dy;  dgamma = sum dy xh, xh = (a - mean) rstd in fp32;  both sums in double in that one fixed
 *   order, rounded once;  da = (gamma rstd) ((dy - mb) - xh mg) in fp32 with mb = float(sum dy / M), mg = float(sum dy xh / M).
 * wsc_pool_tf_grad_nhwc / wsc_maxpool_grad_nhwc: the gradient of wsc_pool_tf_nhwc (window 2 / 3, stride 1 / 2, SAME / VALID) and of
 *   wsc_maxpool_nhwc (torch's MaxPool2d(k, stride, pad)) at x_dev [N][H][W][C] (C a multiple of 8) for dy_dev of the pool's output
 *   size -> every element of dx_dev [N][H][W][C], by the tie rule above.  A pixel no window covers (a VALID pool's last row) is +0.0.
 *
 * The tape: wsc_net_cls_tape_plan lists, for a B x H x W input, "input" ([B][H][W][3]); per conv "<state-dict key>" (e.g.
 * "vgg16.layer1.0"), its post-ReLU output; on a BatchNorm net also "<key>.bn", the normalised output, and "<key>.stats"
 * ([1][1][1][2 C]: the {mean, rstd} float pairs); "pool:<i>" -- float32 NHWC at `offset` floats of one buffer of *tape_elems_out
 * floats, each the value the next op read (hi + lo of a two-plane precision); entries start on 256-byte lines and the floats
 * between them are not written; max_entries = 0 for the count.  Any other net is WSC_ERR_INVALID.
 * wsc_net_forward_cls_train: x_dev float32 [B][3][H][W] -> tape_dev (256-byte aligned) and feat_dev float32 [B][h][w][F], the map
 *   wsc_cls_loss reads.  The convolutions run in the net's precision on the packed weights, with the ReLU epilogue and without the
 *   folded inference affine; BatchNorm takes the batch statistics of wsc_batch_norm_train_nhwc on the taped fp32 output with the
 *   net's gamma / beta and stores into the net's activation type through the store of the GroupNorm heads (the same fmaf; an
 *   IEEE-half plane that saturates raises the range flag).  run_dev: NULL, or the running statistics of all BatchNorm layers in
 *   stack order, layer l's [2][C_l] block behind those of the layers before it, updated in place.  On a net without BatchNorm the
 *   launches and the bits of feat_dev are wsc_net_forward_features'.  WSC_ERR_INVALID before any launch: a net of another arch, a
 *   NULL pointer, a tape size other than the plan's, keep outside [0, 1], unbiased other than 0 / 1, `unbiased` with a BatchNorm
 *   layer whose map is 1 x 1 at B = 1.
 * wsc_cls_grad: the rotated fp32 kernels of the data-gradient convolutions (packed once from `weights`, the list wsc_net_create
 *   took; a tensor that is not the net's is WSC_ERR_SHAPE naming the layer) and the backward workspace (grown on demand; it belongs
 *   to the stream of the ctx the object was created on).  The net must outlive the object.  wsc_cls_grad_layout: ONE ENTRY PER
 *   PARAMETER in net.common.plain_module_order, under state-dict names -- per conv `<key>.weight`, `<key>.bias`, then its
 *   BatchNorm's `<bn>.weight`, `<bn>.bias`.  A conv weight has kh = kw = 3, its Cin / Cout, w_off its first float and b_off = -1;
 *   it lies as [3][3][Cin][Cout] (what the GEMM writes: torch's [Cout][Cin][3][3] transposed).  A vector has kh = kw = 0, Cin = 0,
 *   Cout its length, b_off its first float and w_off = -1 (the convention of wsc_irn_grad_layout).  No gaps.  The classifier's
 *   Linear has no entry: its gradient is wsc_cls_loss's.
 * wsc_net_backward_cls: dfeat_dev float32 [B][h][w][F] -> every element of grad_dev (16-byte aligned both).  Asynchronous on the
 *   ctx stream (the first call at a larger size allocates the workspace).  A ctx other than the object's, a tape or gradient size
 *   other than the plan's / the layout's is WSC_ERR_INVALID before any launch.  Two calls give the same bits. */
int wsc_batch_norm_train_nhwc(wsc_ctx *ctx, const float *a_dev, long long M, int C, const float *gamma_dev, const float *beta_dev, float eps,
                              float keep, int unbiased, float *run_dev /* [2][C] or NULL */, float *stats_dev /* [C][2] */, float *y_dev);
int wsc_batch_norm_grad_nhwc(wsc_ctx *ctx, const float *a_dev, const float *stats_dev, const float *gamma_dev, const float *dy_dev, long long M,
                             int C, float *da_dev, float *dgamma_dev, float *dbeta_dev);
int wsc_pool_tf_grad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int C, int k, int stride, int same,
                          float *dx_dev);
int wsc_maxpool_grad_nhwc(wsc_ctx *ctx, const float *x_dev, const float *dy_dev, int N, int H, int W, int C, int k, int stride, int pad,
                          float *dx_dev);
int wsc_net_cls_tape_plan(wsc_ctx *ctx, const wsc_net *net, int B, int H, int W, wsc_tape_entry *entries_out, int max_entries, int *n_out,
                          long long *tape_elems_out);
int wsc_net_forward_cls_train(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float keep, int unbiased,
                              float *run_dev /* or NULL */, float *tape_dev, long long tape_elems, float *feat_dev);
typedef struct wsc_cls_grad wsc_cls_grad;
int wsc_cls_grad_create(wsc_ctx *ctx, const wsc_net *net, const wsc_tensor_desc *weights, int n_weights, wsc_cls_grad **out);
void wsc_cls_grad_destroy(wsc_cls_grad *g);
int wsc_cls_grad_layout(const wsc_cls_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *grad_elems_out);
int wsc_net_backward_cls(wsc_ctx *ctx, wsc_cls_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                         const float *dfeat_dev, float *grad_dev, long long grad_elems);

/* ---- 01_train: the dropout sites of the plain stacks (nn.Dropout(p=0.5), common_cnn.py:133-134) ----------------------------------
 * The contract is the one of the SEC / DSRG sites above (wsc_seg_dropout_f32's block), restated: PARITY WITH TENSORFLOW'S AND
 * KERAS' RANDOM STREAMS IS UNPINNED -- their generators are not reproduced.  A keep-mask depends on (seed, step, site, element
 * index) alone.
 *   mask    element i, the linear NHWC index of the site's [B][h][w][C] tensor, draws Philox4x32-10 with key (seed low, seed high)
 *           and counter (low(i >> 2), high(i >> 2), step, site) and takes output word i & 3; u = float(word >> 8) 2^-24; keep iff
 *           u >= drop_prob in fp32
 *   value   d = fmul_rn(y, scale) where kept, +0.0 where dropped; scale = 1.0f / (1.0f - drop_prob); 0 <= drop_prob < 1 (NaN:
 *           WSC_ERR_INVALID); 0 <= step < 2^32
 *   sites   numbered by the order of the 'D' entries of the stack's table (net/vgg16.py:44, net/m7.py:41).  VGG16: site 0 behind
 *           layer5's first entry, site 1 behind its second.  M7: site 0 behind the layer3_p2 pool of the classifier branch
 *   where   on the value the next op reads.  On a BatchNorm net y is the fp32 fma((a - mean) rstd, gamma, beta) of
 *           wsc_batch_norm_train_nhwc: it is dropped and scaled in fp32 and then stored ONCE into the net's activation type
 *           (the two-plane split and the range flag of the un-dropped BatchNorm store); the tape entry "<key>.bn" is the fp32 value
 *           those planes hold.  On a net without BatchNorm (the ADP VGG16) the post-ReLU entry "<key>" is dropped, exactly as
 *           fc6 / fc7 are.  M7's pooled map is dropped as fp32.  The tape plan (wsc_net_cls_tape_plan) does not change: no mask entry
 *   back    a site behind a BatchNorm cannot take its mask from the tape (a kept output may be negative or exactly 0.0): the
 *           gradient kernels REGENERATE the keep bits from (seed, step, site).  A post-ReLU site uses scale [tape > 0], as fc6 / fc7.
 *           M7's site sits in front of the global max: a dropped +0.0 can win the maximum of a channel whose kept values are all
 *           negative; wsc_cls_loss then hands its gradient to that element, and the site's backward makes it +0.0
 *
 * wsc_batch_norm_train_drop_nhwc: wsc_batch_norm_train_nhwc with y_dev = the dropped fp32 output; the statistics and the running
 *   statistics are those of the un-dropped call, bit for bit.  y_dev may lie off the 16-byte grid (4-byte aligned: the scalar form,
 *   the same bits).  At drop_prob = 0 the kernel keeps everything and scale = 1: y_dev has the un-dropped bits.
 * wsc_batch_norm_grad_drop_nhwc: wsc_batch_norm_grad_nhwc where dy_dev is the gradient BEHIND the dropout: both kernels replace
 *   dy on load by keep ? fmul_rn(dy, scale) : +0.0 -- the bits of the un-dropped call on a dy masked that way; no buffer, no pass.
 *   Both: site < 0, drop_prob outside [0, 1) or NaN, step outside [0, 2^32) and everything the un-dropped entries refuse are
 *   WSC_ERR_INVALID before any launch.
 * wsc_net_cls_feat_dims: the h x w of feat_dev / dfeat_dev for an H x W input.  With `dropping` (non-zero: drop_prob > 0) an M7
 *   net's map is the dropped layer3_p2 map [B][hp][wp][F], which the global max of wsc_cls_loss then reduces; a VGG16 net's stays
 *   [B][h][w][F], then the dropped output of site 1.  dropping = 0: the last feature map of either net.
 * wsc_net_forward_cls_train_drop / wsc_net_backward_cls_drop: the two passes with the sites active.  feat_elems / dfeat_elems: the
 *   floats of feat_dev / dfeat_dev, B h w F of wsc_net_cls_feat_dims(dropping = drop_prob > 0); any other value is
 *   WSC_ERR_INVALID, as are the dropout arguments above and everything the un-dropped entry points refuse -- all before any launch.
 *   AT drop_prob = 0 BOTH ISSUE THE LAUNCHES OF wsc_net_forward_cls_train / wsc_net_backward_cls AND GIVE THEIR BITS (M7: the
 *   un-pooled feature map and its size).  At a BatchNorm site one kernel replaces the apply-and-copy pair of the forward pass; M7
 *   adds the pool, the fp32 copy and wsc_seg_dropout_f32's kernel forward, that kernel on dfeat_dev and the pool gradient backward.
 *   wsc_net_backward_cls_drop MUST BE GIVEN THE (drop_prob, seed, step) OF THE FORWARD PASS THAT WROTE THE TAPE: nothing on the tape
 *   records them, and other values give the gradient of another mask without any error. */
int wsc_batch_norm_train_drop_nhwc(wsc_ctx *ctx, const float *a_dev, long long M, int C, const float *gamma_dev, const float *beta_dev, float eps,
                                   float keep, int unbiased, float *run_dev /* [2][C] or NULL */, float *stats_dev /* [C][2] */, float *y_dev,
                                   float drop_prob, unsigned long long seed, long long step, int site);
int wsc_batch_norm_grad_drop_nhwc(wsc_ctx *ctx, const float *a_dev, const float *stats_dev, const float *gamma_dev, const float *dy_dev,
                                  long long M, int C, float *da_dev, float *dgamma_dev, float *dbeta_dev, float drop_prob,
                                  unsigned long long seed, long long step, int site);
int wsc_net_cls_feat_dims(const wsc_net *net, int H, int W, int dropping, int *h, int *w);
int wsc_net_forward_cls_train_drop(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int B, int H, int W, float keep, int unbiased,
                                   float *run_dev /* or NULL */, float *tape_dev, long long tape_elems, float *feat_dev, long long feat_elems,
                                   float drop_prob, unsigned long long seed, long long step);
int wsc_net_backward_cls_drop(wsc_ctx *ctx, wsc_cls_grad *g, int B, int H, int W, const float *tape_dev, long long tape_elems,
                              const float *dfeat_dev, float *grad_dev, long long grad_elems, long long dfeat_elems, float drop_prob,
                              unsigned long long seed, long long step);

/* ---- 01_train: the update half of a step -- Keras' SGD with Nesterov momentum and the repack of the updated parameters ----------
 * wsc_cls_param_layout: the TRAINING layout of a wsc_cls_grad.  Every entry of wsc_cls_grad_layout, unchanged and at the same
 *   offsets (wsc_cls_grad_layout and its grad_elems do not change); then `<root>.classifier.0.weight` (kh = kw = 1, Cin = F,
 *   Cout = C, w_off = grad_elems): the C rows of the Linear the net uses, lying as torch's [C][F] -- THE ONE MATRIX OF THE LAYOUT
 *   THAT IS NOT IN [Cin][Cout] ORDER, because that is how wsc_cls_loss reads w_dev and writes grad_w_dev; then
 *   `<root>.classifier.0.bias` (a vector entry, b_off = grad_elems + C F) if the net has one.  No gaps; *param_elems_out =
 *   grad_elems + C F [+ C].  max_entries = 0 for the count.
 *   Parameters, gradient and momentum are each ONE fp32 device buffer of param_elems floats in this layout, element for element.
 *   wsc_net_backward_cls writes the first grad_elems floats of such a gradient buffer, wsc_cls_loss writes grad_w_dev /
 *   grad_bias_dev straight into its tail, and reads w_dev / bias_dev from the tail of the parameter buffer.  ALIGNMENT: grad_elems
 *   is a multiple of 64 (every conv has Cout % 64 == 0, the first one 27 x 64 weights) and F a multiple of 4, so in a 16-byte
 *   aligned buffer the front (wsc_net_backward_cls: grad_dev 16-byte aligned) and the classifier weight (wsc_cls_loss: w_dev and
 *   grad_w_dev 16-byte aligned) are on the 16-byte grid for every C -- C = 20 and C = 5 alike (5 x 1024 and 5 x 256 are multiples
 *   of 4); the bias behind it is 16-byte aligned too, and needs only its 4 bytes (bias_dev / grad_bias_dev have no alignment rule).
 *
 * wsc_cls_sgd_step: Keras 2.2's optimizers.SGD(lr, momentum, decay=0.0, nesterov).get_updates (01_train/demo.py:60: momentum 0.9,
 *   nesterov=True), per element
 *     v = momentum m - lr g;   m = v
 *     p = (p + momentum v) - lr g          (nesterov = 1)
 *     p = p + v                            (nesterov = 0)
 *   every product, sum and difference one fp32 rounding in exactly this association (no fused multiply-add), lr g formed ONCE and
 *   used in both places; one rate for every parameter, no weight decay; a momentum buffer of +0.0 gives the first step.  The
 *   schedule (cls_train.step_lr / cyclic_lr) is the caller's.  One launch on 16-byte vectors; buffers off the 16-byte grid take the
 *   scalar form of the same kernel, the same roundings.  grad_dev is only read.  A NaN gradient makes p and m NaN at that element
 *   and nowhere else.  Asynchronous on the ctx stream.  WSC_ERR_INVALID before any launch: ctx is not the context of `g`, elems is
 *   not param_elems, a null pointer, lr negative or not finite, momentum outside [0, 1), nesterov other than 0 / 1.
 *
 * wsc_net_cls_load_params: the counterpart of wsc_net_seg_load_params / wsc_net_irn_load_params.  Rewrites, in place and without a
 *   host copy, everything derived from the parameters, from the floats of param_dev (the training layout):
 *   (a) of every conv of the stack the packed rows in the kernel's K order for the net's precision with s1 and the bias (IEEE-half
 *       modes: the per-output-channel power-of-two scale from the channel's largest |w|; split modes: both parts; fp32 in
 *       WSC_PREC_F32), the first layer's small form included;
 *   (b) the device gamma / beta of every BatchNorm (what wsc_net_forward_cls_train and wsc_net_backward_cls read);
 *   (c) on a BatchNorm net each conv's inference epilogue s2 / b2 from gamma, beta, the layer's eps and run_dev, the running
 *       statistics in the layout wsc_net_forward_cls_train updates ([2][C_l] per layer in stack order): sc = gamma / sqrt(var + eps),
 *       b = beta - mean sc in double -- wsc_net_create's fold, operation for operation, with the correctly rounded double division
 *       and square root -- each rounded to float once.  run_dev = NULL leaves s2 / b2 as they are; a net without BatchNorm ignores
 *       run_dev;
 *   (d) the classifier's fp32 weight and bias, and on a VGG16 net the CAM head's packed rows (the Linear as a 1 x 1 conv; the
 *       [C][F] matrix is transposed into a buffer of the wsc_cls_grad first).  An M7 net's head is its `gradcam_weights` tensor,
 *       which is no parameter of this layout: it stays as it is;
 *   (e) in the wsc_cls_grad the rotated fp32 data-gradient kernels.
 *   Afterwards the device bytes of both objects are what wsc_net_create / wsc_cls_grad_create make of the same floats and running
 *   statistics (M7: and the same `gradcam_weights`).  A parameter, scale or shift that is not finite raises the range flag.
 *   The call WRITES the net, with the ordering caveat of wsc_net_seg_load_params: the net must not be in use on another stream
 *   during it, and work of other streams that reads the net must be ordered behind it by the caller (wsc_ctx_wait).  A handful of launches whatever the depth: the job
 *   tables are built by the first call.  WSC_ERR_INVALID before any launch: a net that is no WSC_ARCH_VGG16_CAM /
 *   WSC_ARCH_M7_CAM net, a `g` of another net, a foreign ctx, a wrong elems, a null param_dev, a VGG16 net built with
 *   `gradcam_weights` (its head is not the classifier).  Asynchronous on the ctx stream. */
int wsc_cls_param_layout(const wsc_cls_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *param_elems_out);
int wsc_cls_sgd_step(wsc_ctx *ctx, wsc_cls_grad *g, float *param_dev, const float *grad_dev, float *mom_dev, long long elems, float lr,
                     float momentum, int nesterov);
int wsc_net_cls_load_params(wsc_ctx *ctx, wsc_net *net, wsc_cls_grad *g, const float *param_dev, long long elems,
                            const float *run_dev /* or NULL */);

/* One 01_train batch of network inputs from decoded uint8 RGB images (csrc/cls_batch.hip): what Keras' ImageDataGenerator behind
 * flow_from_dataframe(target_size=(H, W)) does to a sample (the generators of 02_cues/dataset.py:28-96 and 03c_hsn/dataset.py;
 * 01_train/demo.py:56,100-124 trains on them), in Keras' order, for given random choices --
 *   1. resize       load_img: PIL Image.resize((W, H), NEAREST), skipped when the image is H x W already; the index tables of
 *                   wsc_pil_resize_u8's order 0, built on the host.  The resized image is never written: every tap below reads the
 *                   source through the tables.
 *   2. warp         where bit 0 of the sample's flags is set: scipy.ndimage.affine_transform(plane, M, off, order=1, mode, cval)
 *                   on each float32 H x W plane, in double and in scipy's order of operations (ni_interpolation.c):
 *                     c_k = 0; c_k += row M[k][0]; c_k += col M[k][1]; c_k += off[k]   (k = 0 the row axis; the offset is
 *                     added LAST), mapped by the mode;
 *                     c_k <= -1 (constant mode outside the image): cval;  else start = floor(c_k), f = c_k - start,
 *                     w0 = 1 - f, w1 = 1 - w0, both tap indices mapped by the mode again (nearest and constant: a clamp),
 *                     t = 0; t += (v[i][j] wy[i]) wx[j] in (i, j) order; ONE rounding to float32.
 *                   fill_mode WSC_CLS_FILL_NEAREST / _REFLECT (scipy's grid reflection d c b a | a b c d) / _CONSTANT.  scipy's
 *                   'wrap' is WSC_ERR_INVALID: no reference generator uses it.
 *   3. flips        flip_axis on the columns (bit 1) and / or the rows (bit 2), AFTER the warp
 *   4. standardise  preprocessing_function, then rescale: y = ((v - sub[c]) / div) * mul, each operation one fp32 rounding.
 *                   ADP: sub = 193.09203 on every channel, div = float32(56.450138 + 1e-7), mul = 1; VOC2012: sub = (104, 117, 123)
 *                   on R, G, B as the reference writes it, div = 1, mul = float32(1 / 255); DeepGlobe: sub = 0, div = 1,
 *                   mul = float32(1 / 255)
 *   5. HWC -> CHW   the channels stay R, G, B (what cues.utilities._to_nchw feeds the same nets)
 * Equal to PIL 12 + scipy 1.15 + numpy on every bit: tests/test_cls_batch_oracle.py pins the numpy restatement
 * tests/cls_batch_ref.py against them, tests/test_gpu_cls_batch.py the kernel against the restatement.
 *   images_dev uint8: sample b's image [H_b][W_b][3] at byte offset_host[b];  size_hw_host int32 [B][2];
 *   affine_host double [B][6]: M00 M01 M10 M11 off0 off1, axis 0 = the row (read only where bit 0 of the flags is set);
 *   flags_host int32 [B]: bit 0 warp, bit 1 flip columns, bit 2 flip rows;  sub3_host float [3];
 *   x_dev float32 [B][3][H][W].  One launch; 16-byte stores over the flat output when x_dev is 16-byte aligned, the same
 *   arithmetic in scalar stores otherwise and for the last (B 3 H W) % 4 floats.  Asynchronous on the ctx stream; the staged
 *   table is the only scratch.
 * WSC_ERR_INVALID, naming the sample and before any launch: a matrix or offset that is not finite; a warp that maps one of the
 * four output corners further than 2^20 pixels from the image (the integer conversions of the reflection stay defined); div = 0
 * or a standardisation constant or cval that is not finite; B outside 1 .. 65535; H or W outside 1 .. 32768; a source side
 * outside 1 .. 32768; a negative offset; flag bits above bit 2; an unknown fill_mode; a null pointer. */
#define WSC_CLS_FILL_NEAREST 0
#define WSC_CLS_FILL_REFLECT 1
#define WSC_CLS_FILL_CONSTANT 2
#define WSC_CLS_FLAG_WARP 1
#define WSC_CLS_FLAG_FLIP_COLS 2
#define WSC_CLS_FLAG_FLIP_ROWS 4
int wsc_cls_train_batch(wsc_ctx *ctx, const uint8_t *images_dev, int B, const int32_t *size_hw_host, const int64_t *offset_host,
                        int H, int W, const double *affine_host /* [B][6] */, const int32_t *flags_host /* [B] */,
                        int fill_mode /* WSC_CLS_FILL_* */, float cval, const float *sub3_host, float div, float mul, float *x_dev);

/* ---- backward pass of the IRNet heads: total_loss.backward() of step/train_irn.py:127 ------------------------------------------
 * Net.forward detaches every backbone stage (resnet50_irn.py:111-115) and trainable_parameters() is edge_layers + dp_layers, so
 * the gradient of the heads is the whole gradient of a step.  wsc_irn_aff_loss hands out d total / d edge_out and d total /
 * d dp_out; wsc_net_backward_edge carries them to every head parameter in exact fp32 / double whatever the net's forward
 * precision.  The definition is the chain rule EVALUATED AT THE TAPE: a ReLU passes its gradient where the taped concat value is
 * > 0 (an exact 0 masks); the bilinear upsample's adjoint uses the float weights of the forward kernel, both taps counting where
 * they land on one source pixel; the crop drops what lies outside; GroupNorm's backward takes xh = (z - mean) rstd from the taped
 * z and the taped float {mean, rstd}; stage taps receive no gradient; each concat buffer has one reader, so its gradient is
 * written whole and never accumulated.
 *
 * The tape: wsc_net_edge_tape_plan lists, for N samples of S x S, every stage tap a head reads ("x<k>", [N][H][W][C]), per head
 * its conv output ("<head>.z", [N][ho][wo][Cout]) and its GroupNorm statistics ("<head>.stats", [N][1][1][2 G]: the {mean, rstd}
 * float pairs of the forward pass), and every concat buffer ("cat<i>", [N][Hc][Wc][Ctot], padding channels included) -- float32
 * at `offset` floats of one buffer of *tape_elems_out floats, each the value the next op read (hi + lo of a two-plane precision);
 * entries start on 256-byte lines and the floats between them are not written.  max_entries = 0 for the count.
 * wsc_net_forward_edge_tape is wsc_net_forward_edge_raw (the same launches, the same bits in edge_dev / dp_dev) with a head's conv
 * and statistics written straight into their entries and the taps and concat buffers copied.  tape_dev starts on a 256-byte line.
 *
 * wsc_irn_grad: the rotated fp32 kernels of the data-gradient convolutions (packed once) and the backward workspace (grown on
 * demand; it belongs to the stream of the ctx the object was created on).  `weights`: the list wsc_net_create took; a head tensor
 * that is not the net's is WSC_ERR_SHAPE naming the layer.  The net must outlive the object.  wsc_irn_grad_layout: ONE ENTRY PER
 * PARAMETER in the order of trainable_parameters() -- the heads of edge_layers (`<head>.0.weight`, `<head>.1.weight`,
 * `<head>.1.bias`), the final edge conv's `.weight` / `.bias`, the heads of dp_layers, the final displacement conv's `.weight` --
 * under their state-dict names.  A conv weight has kh = kw = 1, its Cin / Cout, w_off its first float and b_off = -1; it lies as
 * [Cin][Cout] (what the GEMM writes: the transpose of torch's [Cout][Cin][1][1]).  A vector (GroupNorm weight / bias, conv bias)
 * has kh = kw = 0, Cin = 0, Cout its length, b_off its first float and w_off = -1.  No gaps; the padding channels of a concat
 * buffer (160 -> 192) have no entry.
 *
 * wsc_net_backward_edge: dedge_dev float32 [N][He][We], ddp_dev float32 [N][2][Hd][Wd] (the layouts wsc_irn_aff_loss writes) ->
 * every element of grad_dev.  Asynchronous on the ctx stream (the first call at a larger size allocates the workspace).  A net
 * that is no IRNet net, a ctx other than the object's, a tape or gradient size other than the plan's / the layout's is
 * WSC_ERR_INVALID before any launch.  Two calls give the same bits: no floating-point atomic, every sum in one fixed order.
 *
 * The two new kernels one by one, for the per-op tests (float32 NHWC, the pass's own launchers unchanged):
 * wsc_relu_upsample_grad_nhwc: dy_dev [N][H][W][C] = the adjoint of "upsample by up (1, 2, 4), crop to Hd x Wd, ReLU, write
 *   channels [coff, coff + C) of [N][Hd][Wd][Ctot]" applied to dcat_dev, masked by cat_dev > 0 (both [N][Hd][Wd][Ctot]).
 * wsc_group_norm_grad_nhwc: dz_dev [N][H][W][C], dgamma_dev [C], dbeta_dev [C] of nn.GroupNorm(G, C) at input z_dev and output
 *   gradient dy_dev; gamma_host [C]; the statistics are formed as the forward pass forms them (float {mean, rstd}). */
int wsc_net_edge_tape_plan(wsc_ctx *ctx, const wsc_net *net, int N, int S, wsc_tape_entry *entries_out, int max_entries, int *n_out,
                           long long *tape_elems_out);
int wsc_net_forward_edge_tape(wsc_ctx *ctx, const wsc_net *net, const float *x_dev, int N, int S, float *tape_dev, long long tape_elems,
                              float *edge_dev, float *dp_dev);
typedef struct wsc_irn_grad wsc_irn_grad;
int wsc_irn_grad_create(wsc_ctx *ctx, const wsc_net *net, const wsc_tensor_desc *weights, int n_weights, wsc_irn_grad **out);
void wsc_irn_grad_destroy(wsc_irn_grad *g);
int wsc_irn_grad_layout(const wsc_irn_grad *g, wsc_grad_entry *entries_out, int max_entries, int *n_out, long long *grad_elems_out);
int wsc_net_backward_edge(wsc_ctx *ctx, wsc_irn_grad *g, int N, int S, const float *tape_dev, long long tape_elems, const float *dedge_dev,
                          const float *ddp_dev, float *grad_dev, long long grad_elems);
int wsc_relu_upsample_grad_nhwc(wsc_ctx *ctx, const float *dcat_dev, const float *cat_dev, int N, int H, int W, int C, int up, int Hd, int Wd,
                                int Ctot, int coff, float *dy_dev);
int wsc_group_norm_grad_nhwc(wsc_ctx *ctx, const float *z_dev, const float *dy_dev, int N, int H, int W, int C, const float *gamma_host, int G,
                             float eps, float *dz_dev, float *dgamma_dev, float *dbeta_dev);

/* ---- the update half of an IRNet training step and the closing dp_mean pass (step/train_irn.py:86-90, 127-129, 148-164) ---------
 * Parameters, gradient and momentum are each ONE fp32 device buffer of grad_elems floats in the layout of wsc_irn_grad_layout,
 * element-for-element parallel.  train_irn.py:86-90 builds PolyOptimizer with two groups: param_groups[0] (edge_layers: every
 * `fc_edge*` entry, the layout's leading ones) at lr, param_groups[1] (dp_layers: the rest) at 10 lr, one weight decay.
 *
 * wsc_irn_sgd_step: optimizer.step() of lines 127-129, torch.optim.SGD with dampening 0 and no Nesterov, per element
 *     g = grad + weight_decay p       (every parameter: conv weights, GroupNorm weight AND bias, the edge conv's bias)
 *     m = sgd_momentum m + g          (a momentum buffer that starts at +0.0 gives torch's first step, m = g)
 *     p = p - lr_group m              lr_group = lr_edge before the first dp entry's offset, lr_dp from there on
 *   every product and sum rounded to fp32 on its own (no fused multiply-add), the same roundings in the 16-byte form and in the
 *   scalar form an unaligned buffer takes.  The poly schedule lr0 (1 - step / max_step)^power is the caller's (evaluated in
 *   double on the host and rounded to float, as torch does for fp32 tensors).  One launch, asynchronous on the ctx stream;
 *   grad_dev is only read.  WSC_ERR_INVALID before any launch: ctx is not the context of `g`, elems is not the layout's
 *   grad_elems, a null pointer, a scalar that is not finite.
 *
 * wsc_net_irn_load_params: the counterpart of wsc_net_seg_load_params.  Rewrites, in place and without a host copy, everything
 * derived from the head parameters, from the floats of param_dev: (a) of every head the packed conv rows in the kernel's K order
 * for the net's precision with the epilogue scale (IEEE-half modes: the per-output-channel power-of-two scale from the channel's
 * largest |w|; split modes: both parts; fp32 in WSC_PREC_F32) and its device GroupNorm weight / bias; (b) the final edge conv (its
 * edge_in = 160 input channels inside a row padded to the edge concat's 192, the padding exact zeros, its bias) and the final
 * displacement conv; (c) in the wsc_irn_grad the rotated fp32 data-gradient kernels of the heads that read a concat buffer and of
 * the two final convs.  Afterwards the device bytes of both objects are what wsc_net_create and wsc_irn_grad_create make of the
 * same floats.  mean_shift is not a parameter: wsc_net_set_mean_shift.  The call WRITES the net, with the ordering caveat of
 * wsc_net_seg_load_params.  WSC_ERR_INVALID before any launch: a net that is no IRNet net, a `g` of another net, a foreign ctx,
 * a wrong elems.  Asynchronous on the ctx stream, a handful of launches whatever the number of heads.
 *
 * wsc_channel_mean_nchw: out_dev[c] (double, 8-byte aligned) = mean over (n, h, w) of x_dev [N][C][H][W] (float32) in double,
 * minus sub_host[c] (float, NULL: nothing) -- torch.mean(dp, dim=(0, 2, 3)) of train_irn.py:158 with MeanShift's eval-mode
 * subtraction of running_mean.  Per-block partial sums in one fixed order, the last block of a channel to arrive (an integer
 * ticket) adds them in block order: no floating-point atomic, two calls give the same bits.  C <= 1024.  Asynchronous.
 *
 * wsc_net_set_mean_shift / wsc_net_get_mean_shift: the two floats (mean_shift.running_mean, train_irn.py:164) that
 * wsc_net_forward_edge subtracts from dp; host state of the net, read when a forward call is enqueued. */
int wsc_irn_sgd_step(wsc_ctx *ctx, wsc_irn_grad *g, float *param_dev, const float *grad_dev, float *mom_dev, long long elems, float lr_edge,
                     float lr_dp, float weight_decay, float sgd_momentum);
int wsc_net_irn_load_params(wsc_ctx *ctx, wsc_net *net, wsc_irn_grad *g, const float *param_dev, long long elems);
int wsc_channel_mean_nchw(wsc_ctx *ctx, const float *x_dev, int N, int C, int H, int W, const float *sub_host /* [C] or NULL */,
                          double *out_dev /* [C] */);
int wsc_net_set_mean_shift(wsc_net *net, const float m[2]);
int wsc_net_get_mean_shift(const wsc_net *net, float m_out[2]);

/* ---- 02_cues: the localization seeds SEC / DSRG train on (02_cues/utilities.py:183-278 get_localization_cues /
 * get_localization_cues_sec, 02_cues/adp_cues.py:304-339 update_cues; consumer 03a_sec-dsrg/model.py:238-246) ---- */

/* The gated, channel-selected, resized Grad-CAM stack, from the NHWC maps of wsc_net_forward_gradcam in place:
 *   out[b][c] = bilinear(cams[b][:, :, chan[c]] * gate[b][c])  to S x S
 * -- exactly the bits of "multiply by the 0/1 gate on the host, transpose NHWC -> NCHW, wsc_bilinear_resize" (one sampler,
 * csrc/bilerp.h; the gate is a multiplication here too, so a gated negative value is -0 on both paths).
 *   cams_nhwc_dev float32 [B][h][w][C_all];  chan_host int32 [C], each in [0, C_all);  gate_dev float32 [B][C] or NULL (all 1);
 *   out_dev float32 [B][C][S][S]. */
int wsc_cue_maps(wsc_ctx *ctx, const float *cams_nhwc_dev, int B, int h, int w, int C_all, const int32_t *chan_host, int C,
                 const float *gate_dev, int S, float *out_dev);

/* Seed label maps of a batch.  The localization stack has L = C + (bg_dev != NULL) channels; with bg_dev channel 0 is the
 * background and foreground class c is channel c + 1, else class c is channel c.
 *   foreground mask of class c: (double)fg[b][c][p] > thresh * (double)max_c, product and comparison in double as numpy forms
 *     them from a Python-float thresh and float64 maps.  max_c is the maximum of class c over the WHOLE BATCH when
 *     per_image_max == 0 (utilities.py:218,262 -- SURVEY Q7), over image b's own map when per_image_max != 0
 *     (adp_cues.py:322-323).  Maps of either sign are legal (the ADP background channel can be <= 0 everywhere); a class whose
 *     maximum is 0 has an empty mask.
 *   background mask: s[p] = sum_k (double)bg[b][k][p], added sequentially in channel order from 0 (np.sum(axis=0) of the float64
 *     stack); m = 3 x 3 median of s with scipy.ndimage's default mode='reflect' border (the edge sample is repeated); the mask
 *     is m[p] < sorted(m)[int(bg_fraction * H * W)], strict -- a constant plane yields no background seed.
 *   overlap resolution: the area of a channel is the pixel count of its mask; label[b][p] = k + 1 for the covering channel k of
 *     the smallest area, 0 where no mask covers the pixel.  TIE RULE: among covering channels of equal area the HIGHER channel
 *     index wins -- "visit the masks from the largest to the smallest, each paints over what is there" under
 *     np.argsort(-area, kind='stable').  The reference calls np.argsort(-area) with the default kind, whose order among equal
 *     areas is unspecified; its result on such pixels is not a contract.
 *   fg_dev float32 [B][C][H][W];  bg_dev float32 [B][Cb][H][W] or NULL;  label_dev uint8 [B][H*W];
 *   area_dev int32 [B][L] or NULL: the mask areas.  The inputs are not modified.
 * Limits, checked before any launch (WSC_ERR_INVALID): 1 <= L <= 32; H * W <= 4096 (an image's planes live in LDS; the
 * reference's maps are 41 x 41); B, C, H, W >= 1 and Cb >= 1 with bg_dev; 0 <= bg_fraction < 1; only bg_dev and area_dev may be
 * NULL.  NaN inputs are out of contract. */
int wsc_cue_seeds(wsc_ctx *ctx, const float *fg_dev, const float *bg_dev, int B, int C, int Cb, int H, int W, double thresh,
                  int per_image_max, double bg_fraction, uint8_t *label_dev, int32_t *area_dev);

/* ---- SEC / DSRG prediction tail (03a_sec-dsrg/model.py:665-719): eval_miou with is_eval=True, the glue around the dense CRF ----
 * Both calls take a ragged batch packed back to back with host offset arrays (the convention of wsc_sem_seg_finish and
 * wsc_label_confusion_nn) and run as ONE launch over the batch.  The resize is the sampler of wsc_bilinear_resize
 * (csrc/bilerp.h: half-pixel centres, clamped, separate fp32 scales h/H and w/W), so a resized value has the bits that
 * wsc_bilinear_resize gives for that class plane, and equal source and output sizes pass the map through unchanged (weights
 * exactly 1 and 0).  That rule is cv2's INTER_LINEAR rule (csrc/hsn.hip); cv2 itself is absent offline, parity with its
 * float arithmetic is unpinned.
 * Limits, checked before any launch (WSC_ERR_INVALID): 1 <= C <= 32; 1 <= B <= 65535; every size >= 1 and every image's pixel
 * count within int32; no NULL pointer. */

/* cv2.resize(prob, (W, H)) followed by the unary of lib.crf.crf_inference(use_log=True)  (model.py:686,689):
 *   U[b][c][p] = -log( bilinear(prob[b][:, :, c])[p] )
 * prob_dev: image b's NHWC block float32 [h_b][w_b][C] at float offset prob_off[b] (as the network's rescale_output leaves it);
 * unary_dev: image b's CLASS-major block float32 [C][H_b*W_b] at float offset unary_off[b] (what wsc_crf_v_inference takes).
 * No clip: the mirror (misc.imutils.crf_inference) takes -log of the map as it is; probabilities must be > 0. */
int wsc_seg_unary_nhwc(wsc_ctx *ctx, const float *prob_dev, int B, int C, const int64_t *prob_off_host /*[B]*/,
                       const int32_t *src_hw_host /*[B][2]*/, const int32_t *out_hw_host /*[B][2]*/,
                       const int64_t *unary_off_host /*[B]*/, float *unary_dev);

/* The DeepGlobe branch's tail (model.py:695 + :699): cv2.resize of the CRF marginals to the ground truth's size, then arg-max over
 * the classes (FIRST maximum, as np.argmax; NaN is out of contract).  q_dev: class-major [C][h_b*w_b] at float offset q_off[b]
 * (wsc_crf_v_inference's q); label_dev int32, H_b*W_b per image at int32 offset label_off[b] (what wsc_label_confusion_nn
 * takes).  The resized marginals are never written. */
int wsc_seg_resize_argmax(wsc_ctx *ctx, const float *q_dev, int B, int C, const int64_t *q_off_host /*[B]*/,
                          const int32_t *src_hw_host /*[B][2]*/, const int32_t *out_hw_host /*[B][2]*/,
                          const int64_t *label_off_host /*[B]*/, int32_t *label_dev);

/* ---- SEC / DSRG: the steps that keep Model.predict (model.py:542-586) and the CRF layer (build_crf) on the device ----------------
 * All four are asynchronous on the ctx stream, copy their host descriptor arrays during the call, and check their limits before
 * any launch (WSC_ERR_INVALID, the text names the argument): no NULL pointer, every size >= 1 (a pixel count within int32),
 * 1 <= C <= 32, 1 <= n / B <= 65535.  The TF resize is wsc_resize_bilinear_tf's, operation for operation (no FMA contraction):
 * a value has the bits that call gives for it, and equal sizes pass through exactly (t == 0). */

/* image_preprocess of the evaluation phases (model.py:332-346) for a ragged batch in ONE launch.
 * img_dev: packed uint8 RGB images, image i's [h_i][w_i][3] block at BYTE offset src_off_host[i], sizes src_hw_host[i] = {h_i, w_i};
 * x_dev float32 [n][H][W][3]:  x[i][y][x][c] = resize_bilinear_tf(float(img_i), (H, W))[y][x][2 - c] - mean_bgr_host[c]  (fp32). */
int wsc_seg_preprocess_u8(wsc_ctx *ctx, const uint8_t *img_dev, int n, const int32_t *src_hw_host /*[n][2]*/,
                          const int64_t *src_off_host /*[n]*/, const float *mean_bgr_host /*[3]*/, int H, int W, float *x_dev);

/* The CRF layer's zoomed image (DSRG.py:318-319,325 / SEC.py build_crf): v = x + mean_host[c] (one fp32 rounding), TF-resized to
 * (sh, sw), then image.astype(np.uint8), DEFINED here as truncation toward zero to int32 and the low 8 bits of that,
 * (uint8_t)(int32_t)v: numpy's result for every in-range value, astype(np.int32).astype(np.uint8) for finite |v| < 2^31.  NaN and
 * larger magnitudes are outside the contract.  The channel order stays as it is.
 * x_dev float32 [B][H][W][3];  out_dev uint8 [B][sh][sw][3] (what wsc_crf_create takes). */
int wsc_seg_crf_image_u8(wsc_ctx *ctx, const float *x_dev, int B, int H, int W, const float *mean_host /*[3]*/, int sh, int sw,
                         uint8_t *out_dev);

/* The tail of the `crf` closure (DSRG.py:329-332): p_c = q_c < min_prob ? min_prob : q_c;  s = the fp32 sum of p_c in class order;
 * out_c = logf(p_c / s).  q_dev float32 [B][C][n] class-major (wsc_crf_inference's q);  out_dev float32 [B][n][C] NHWC. */
int wsc_seg_crf_logprob(wsc_ctx *ctx, const float *q_dev, int B, int C, long long n, float min_prob, float *out_dev);

/* NHWC maps [B][n][C] -> class-major planes [B][C][n], the layout wsc_seg_resize_argmax reads: the is_eval=False pass of eval_miou
 * (model.py:666-669) takes the arg-max of the network's NHWC softmax through that call at equal sizes. */
int wsc_seg_planes_from_nhwc(wsc_ctx *ctx, const float *src_dev, int B, int C, long long n, float *dst_dev);

/* ---- SEC / DSRG: the inputs of a training step and the ground truth of a validation batch (csrc/seg_batch.hip) --------------------
 * Both are asynchronous on the ctx stream, copy their host arrays during the call (one staged table each) and check every limit
 * and every list entry on the host arrays BEFORE any launch: WSC_ERR_INVALID, the text names the sample, nothing is written.
 * Limits: 1 <= B <= 65535, 1 <= C / n_class <= 32, s * s <= 8192, every size >= 1 with a pixel count within int32, byte offsets
 * >= 0, list offsets neither negative nor decreasing. */

/* One training batch of Model.next_batch: m_train / get_data (model.py:229-252) and image_preprocess (:318-331).
 * img_dev, src_hw_host, src_off_host, mean_bgr_host, H, W, x_dev: exactly wsc_seg_preprocess_u8's, which forms x_dev (its bits).
 * cues_host: the (class, row, col) lists of localization_cues.pickle, sample b's [3][n_b] int32 block at int index
 *   3 * cue_off_host[b], n_b = cue_off_host[b + 1] - cue_off_host[b] (0 is legal, duplicates are legal);
 * labels_host: sample b's classes at int index label_off_host[b] .. label_off_host[b + 1].
 * cues_dev float32 [B][s][s][C]: 1.0 where (row, col, class) is listed, 0.0 elsewhere (cues[cues_i[1], cues_i[2], cues_i[0]] = 1.0);
 * labels_dev float32 [B][C]: 1.0 at the listed classes and at class 0 (label[0] = 1.0, :240-242), 0.0 elsewhere.
 * Every element of both is written exactly once by a plain store (no memset, no global atomic).  Two launches. */
int wsc_seg_train_batch(wsc_ctx *ctx, const uint8_t *img_dev, int B, const int32_t *src_hw_host /*[B][2]*/,
                        const int64_t *src_off_host /*[B]*/, const int32_t *cues_host, const int32_t *cue_off_host /*[B+1]*/,
                        const int32_t *labels_host, const int32_t *label_off_host /*[B+1]*/, const float *mean_bgr_host /*[3]*/,
                        int H, int W, int s, int C, float *x_dev, float *cues_dev, float *labels_dev);

/* The ground truth of a validation batch: m_val / image_preprocess (model.py:254-270, :338-342), then the class test of
 * eval_miou (:701, :709-714).  gt_dev: packed uint8 blocks [h_b][w_b][channels] (channels 1 or 3) at BYTE offset src_off_host[b].
 * Resize: TF 1.x resize_nearest_neighbor(align_corners=False), in float32 as TF computes it --
 *   scale = (float)in / (float)out;  src = min((int)floorf((float)dst * scale), in - 1)
 * (tf_tap's scale and product; parity unpinned against TensorFlow, which the project does not install).
 * Class test: colours_host == NULL: channel 0's value k if k < n_class, else n_class (secdsrg.seg_gt_index);
 *   colours_host uint8 [n_class][3]: the first class whose colour equals all three channels, else n_class
 *   (hsn.demo.gt_index_from_colours); a colour table with channels == 1 is WSC_ERR_INVALID.
 * index_dev uint8 [B][OH][OW], values in [0, n_class]. */
int wsc_seg_gt_index_tf(wsc_ctx *ctx, const uint8_t *gt_dev, int B, const int32_t *src_hw_host /*[B][2]*/,
                        const int64_t *src_off_host /*[B]*/, int channels, const uint8_t *colours_host, int n_class, int OH, int OW,
                        uint8_t *index_dev);

/* ---- HistoSegNet post-processing (03c_hsn/utilities.py:231-397), device resident ---------- */

/* HSN grad_cam after the einsum (utilities.py:262-277), for the NHWC maps of wsc_net_forward_gradcam(relu = 0):
 *   per (image, class) cv2.resize(map, (S, S)) (bilinear) then max(., 0); cams /= max(max_{h,w,c} cams, 1e-7) per
 *   image; cams *= gate[b][c]  (gate = conf_scores * is_pass_threshold).
 *   cams_nhwc_dev float32 [B][h][w][C];  gate_dev float32 [B][C];  out_dev float32 [B][C][S*S]  (class-major). */
int wsc_hsn_gradcam_post(wsc_ctx *ctx, const float *cams_nhwc_dev, int B, int h, int w, int C, int S,
                         const float *gate_dev, float *out_dev, int out_channels, int out_first);
/* (out_channels > C: the maps go to channels [out_first, out_first + C) of a wider [B][out_channels][S*S] stack, e.g. behind
 * the background channel of the VOC branch; out_channels <= 0 means a plain [B][C][S*S] output.) */
/* VOC background channel (03c_hsn/demo.py:145-147): X_bg = sum over the bg model's class maps; channel 0 of the stack =
 * 0.15 * expit(max over the WHOLE batch of X_bg - X_bg)  (SURVEY Q6).
 *   Hbg_dev float32 [B][Cb][N];  y_dev float32 [B][Ctot][N] (channel 0 is written). */
int wsc_hsn_voc_background(wsc_ctx *ctx, const float *Hbg_dev, int B, int Cb, int N, float *y_dev, int Ctot);
/* mass[i] = 1 if map i has a positive entry (dcrf_process keeps the classes whose sum is > 0, utilities.py:425; the maps
 * are >= 0).  maps_dev float32 [n_maps][N];  mass_dev uint32 [n_maps]. */
int wsc_hsn_class_mass(wsc_ctx *ctx, const float *maps_dev, int n_maps, int N, uint32_t *mass_dev);
/* modify_by_htt's background activation (utilities.py:341-347; twins 02_cues/adp_cues.py:279-285,
 * 03b_irn/net/common_cam.py:36-44): 0.75 * expit(4 * (mean_rgb - 240)) smoothed by scipy.ndimage.gaussian_filter(
 * sigma = 2) (truncate 4 sigma, mode 'reflect', axis 0 then axis 1), then cv2.resize (bilinear) to Ho x Wo when the
 * CAM grid differs from the image (:345-347).
 *   rgb_dev uint8 [B][H][W][3];  bg_dev FLOAT64 [B][Ho*Wo] (on tissue the activation is far below the fp32 range and
 *   still decides whether the Background class has mass). */
int wsc_hsn_background(wsc_ctx *ctx, const uint8_t *rgb_dev, int B, int H, int W, int Ho, int Wo, double *bg_dev);
/* ADP background / 'other' channels of the 03b_irn CAM networks (03b_irn/net/common_cam.py:31-92, vgg16_cam.py:51-58),
 * joined with the use_cls CAM channels on the device and summed over the scales of an image (make_cam.py:62-69):
 *   mode 0 (adp_morph, :31-55): out[0] = relu(bg - max_k cam[adipose[k]]);  out[1 + i] = cam[use[i]]
 *   mode 1 (adp_func,  :57-92): out[0] = bg - max_k cam[exc[k]];
 *                               out[1] = max(0.05 (1 - max(out[0], max_i cam[use[i]])), max_k cam[adipose[k]]);  out[2 + i] = cam[use[i]]
 *   cam_dev float32 [B][n_sc][C][hw] (wsc_net_forward_cam);  bg_dev float64 [B][n_sc][hw] (wsc_hsn_background of the ORIGINAL,
 *   un-flipped image of each scale, resized to the CAM grid);  use / adipose / exc: channel indices into the C CAM channels
 *   (the caller composes the X1.7 class filter of common_cam.py:26-29 into them);  out_dev float32 [B][n_use + 1 + mode][hw]. */
int wsc_cam_adp_modify(wsc_ctx *ctx, const float *cam_dev, int B, int n_sc, int C, int hw, const double *bg_dev, int mode,
                       const int32_t *use_host, int n_use, const int32_t *adipose_host, int n_adip, const int32_t *exc_host,
                       int n_exc, float *out_dev);
/* The valid-class stack of one HTT type, modify_by_htt (utilities.py:348-363) and get_cs_gradcam (:367-397) in one pass:
 *   Y[v] = H[src_of_valid[v]] (0 where src_of_valid[v] < 0);  Y[bg_ind] = bg - max_{v in exceptions} Y[v];
 *   functional types (other_ind >= 0): Y[other_ind] = max(0.05 * (1 - max_v Y[v]), max_k H[adipose_src[k]]);
 *   cs[v] = (top1 - top2)(Y) where argmax(Y) == v else 0;  cs[other_ind] = Y[other_ind];
 *   mass[b][v] = 1 if cs[b][v] has a positive entry (dcrf_process keeps the classes whose sum is > 0, :425; every
 *   entry of cs is >= 0).
 *   bg_dev == NULL skips the modify_by_htt step (get_cs_gradcam alone on an already modified stack).
 *   H_dev float32 [B][C_all][N] (wsc_hsn_gradcam_post);  bg_dev float64 [B][N];  cs_dev, y_dev (may be NULL) [B][Cv][N];
 *   mass_dev uint32 [B][Cv];  Cv <= 32, at most 4 exception / adipose classes. */
int wsc_hsn_cs_gradcam(wsc_ctx *ctx, const float *H_dev, int B, int C_all, int N, const double *bg_dev,
                       const int32_t *src_of_valid_host, int Cv, int bg_ind, int other_ind,
                       const int32_t *exception_inds_host, int n_exc, const int32_t *adipose_src_host, int n_adip,
                       float *cs_dev, float *y_dev, uint32_t *mass_dev);
/* unary_from_softmax of a gathered channel list (utilities.py:431): unary[i][p] = -log(clip(maps[chan_off[i] + p],
 * 1e-5, 1)), i < n_chan; chan_off_host = float offsets of the channels inside maps_dev. */
int wsc_hsn_gather_unary(wsc_ctx *ctx, const float *maps_dev, const int64_t *chan_off_host, int n_chan, int N,
                         float *unary_dev);

/* ---- dense CRF (pydensecrf replacement) -------------------------------- */

/* DenseCRF2D(W,H,M) + addPairwiseGaussian(sxy=g_sxy) + addPairwiseBilateral(
 * sxy=bi_sxy, srgb=bi_srgb, rgbim) for a batch of B images of one size
 * (03c_hsn/utilities.py:427-440; misc.imutils.crf_inference_label call sites
 * 03b_irn/step/cam_to_ir_label.py:35-67): builds both permutohedral lattices
 * and the symmetric normalisation vectors, which depend on the image only and
 * are reused by every mean-field iteration.
 *   rgb_dev uint8 [B][H][W][3] (HWC, as np.uint8(images[i])). */
int wsc_crf_create(wsc_ctx *ctx, const uint8_t *rgb_dev, int B, int H, int W, float g_sxy,
                   float bi_sxy, float bi_srgb, wsc_crf **out);
/* Ordering rule: the lattice memory goes back to the BUILD ctx's stream-ordered cache.  wsc_crf_inference may run on
 * another ctx (stream); it records the end of its loop in the wsc_crf, and wsc_crf_destroy makes the build ctx's stream
 * wait for that point before any later work of the build ctx can reuse the memory.  The caller only has to keep the
 * wsc_crf alive until wsc_crf_inference has RETURNED (not until it has finished on the device), and must destroy it
 * before the ctx it was created on. */
void wsc_crf_destroy(wsc_crf *crf);
/* number of occupied lattice vertices per image: v_gauss/v_bilat int32[B] host arrays (may be NULL) */
int wsc_crf_lattice_sizes(wsc_ctx *ctx, const wsc_crf *crf, int32_t *v_gauss_host,
                          int32_t *v_bilat_host);
/* 1 when wsc_crf_inference with M classes sums, blurs and slices the Gaussian (addPairwiseGaussian) lattice inside its
 * update kernel -- per pixel tile, in LDS, no value rows in HBM -- and 0 when the separate blur kernel runs (vertex sets of
 * a pixel tile too large for the kernel's LDS at this M: very narrow g_sxy; the first use of an image size on a ctx; or WSC_OPT_CRF_GAUSS_ON_CHIP = 0).  Same Q bits either
 * way; a diagnostic for tests and benchmarks (03c_hsn/utilities.py:435 is the call this concerns). */
int wsc_crf_gaussian_on_chip(const wsc_crf *crf, int M);

/* d.setUnaryEnergy(U); Q = d.inference(n_iters) with Potts compatibilities
 * g_compat / bi_compat (03c_hsn/utilities.py:431-442):
 *   unary_dev float32 [B][M][H*W]  (= -log p, as unary_from_softmax returns it)
 *   q_dev     float32 [B][M][H*W]  or NULL   (np.array(Q))
 *   argmax_dev int32  [B][H*W]     or NULL   (np.argmax(Q, axis=0))
 * M <= 32. */
int wsc_crf_inference(wsc_ctx *ctx, wsc_crf *crf, const float *unary_dev, int M, float g_compat,
                      float bi_compat, int n_iters, float *q_dev, int32_t *argmax_dev);
/* wsc_crf_inference on pixel-major unaries: unary_pm_dev float32 [B][H*W][Mp], Mp = 4 * ceil(M/4), padding classes 0
 * (wsc_cam_unary_pm).  The buffer is read in place during the whole loop and never written. */
int wsc_crf_inference_pm(wsc_ctx *ctx, wsc_crf *crf, const float *unary_pm_dev, int M, float g_compat,
                         float bi_compat, int n_iters, float *q_dev, int32_t *argmax_dev);

/* ---- ragged batch ----------------------------------------------------------------------------------------------------
 * The reference runs its CRF one image at a time, every image with its own size and class count
 * (03b_irn/step/cam_to_ir_label.py:25-58: crf_inference_label per image, K_b + 1 labels; 03c_hsn/utilities.py:420-445:
 * DenseCRF2D(W, H, len(pass_inds[i])) per image).  A wsc_crf_v takes such a list as it comes:
 *   rgb_dev[b]   device pointer of image b, uint8 [H_b][W_b][3];  hw_host[2b], hw_host[2b+1] = H_b, W_b
 * Images of equal size share a lattice build and a mean-field loop; the groups are issued back to back on the ctx's stream
 * (no host synchronisation between them).  wsc_crf_v_inference:
 *   unary_dev[b] device pointer of image b's unaries, float32 [M_b][H_b*W_b] (class-major, as wsc_crf_inference takes them)
 *   M_host[b]    its class count (1..32);  q_dev[b] (float32 [M_b][H_b*W_b]) and / or argmax_dev[b] (int32 [H_b*W_b]);
 *                either pointer ARRAY may be NULL, single entries too
 * Inside a group the loop runs at the largest M_b; a smaller image's missing classes enter with probability zero, which
 * leaves every bit of its result what a call with its own M_b gives (tests/test_gpu_crf.py::test_crf_ragged_batch). */
int wsc_crf_v_create(wsc_ctx *ctx, const uint8_t *const *rgb_dev, const int32_t *hw_host /*[B][2]*/, int B, float g_sxy,
                     float bi_sxy, float bi_srgb, wsc_crf_v **out);
void wsc_crf_v_destroy(wsc_crf_v *crf);
int wsc_crf_v_num_groups(const wsc_crf_v *crf); /* lattice builds / loops the batch needs (distinct image sizes) */
int wsc_crf_v_inference(wsc_ctx *ctx, wsc_crf_v *crf, const float *const *unary_dev, const int32_t *M_host, float g_compat,
                        float bi_compat, int n_iters, float *const *q_dev, int32_t *const *argmax_dev);

#ifdef __cplusplus
}
#endif
#endif /* WSSCAM_H */
