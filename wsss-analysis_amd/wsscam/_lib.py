"""ctypes binding of libwsscam.so (the C ABI of include/wsscam.h).

The product path has no CPU fallback: if the shared library is missing, or no gfx950
device is present, the calls fail loudly (WscError).
"""
import collections
import ctypes
import os
import re
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwsscam.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "wsscam.h"))

WSC_OK = 0
WSC_ERR_INVALID = -1
WSC_ERR_NO_DEVICE = -2
WSC_ERR_HIP = -3
WSC_ERR_MISSING_KEY = -4
WSC_ERR_SHAPE = -5
WSC_ERR_NOMEM = -6
WSC_ERR_KEY_RANGE = -7
WSC_ERR_CAPACITY = -8
WSC_ERR_RANGE = -9  # an IEEE-half activation saturated (|v| >= 65504): the maps are not the reference's fp32 maps

ARCH_RESNET50_CAM = 0
ARCH_VGG16_CAM = 1
ARCH_M7_CAM = 2
ARCH_RESNET50_IRN = 3
ARCH_VGG16_IRN = 4
ARCH_M7_IRN = 5
ARCH_DEEPLAB_LFOV = 6  # SEC: DeepLab-VGG16, one fc6 / fc7 / fc8 branch at rate 12
ARCH_DEEPLAB_ASPP = 7  # DSRG: branches _1 .. _4 at rates 6 / 12 / 18 / 24, fc8 = their sum

PREC_BF16 = 0
PREC_BF16X3 = 1
PREC_F16 = 2
PREC_F16X3 = 3  # split-half operands and activations (hi + lo), three MFMA products: the fp32-class mode
PREC_F32 = 4  # exact fp32 (weights, activations, fp32-input MFMA): the reference's range, the fallback for WSC_ERR_RANGE
# path selectors of a context (include/wsscam.h wsc_option; Context.set_option / Context.option)
OPT_CRF_GAUSS_ON_CHIP, OPT_CRF_FUSED_BLUR, OPT_CRF_BLUR_ON_CHIP, OPT_CRF_RANK_BALLOT, OPT_CRF_EMBED_FULL, OPT_RW_TILED, \
    OPT_STEM_POOL_FUSED, OPT_CONV_WINDOW, OPT_CAM_HEAD_STREAM, OPT_CRF_MSG_IN_UPDATE = range(10)
OPT_DEFAULTS = {OPT_CRF_GAUSS_ON_CHIP: 1, OPT_CRF_FUSED_BLUR: 1, OPT_CRF_BLUR_ON_CHIP: 1, OPT_CRF_RANK_BALLOT: 0,
                OPT_CRF_EMBED_FULL: 0, OPT_RW_TILED: -1, OPT_STEM_POOL_FUSED: 1, OPT_CONV_WINDOW: 1, OPT_CAM_HEAD_STREAM: 1,
                OPT_CRF_MSG_IN_UPDATE: 1}
CONV_GENERIC = 0x100  # conv2d_nchw only: OR into precision to keep the kernel's generic variants (testing)


class WscError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("libwsscam error %d: %s" % (status, message))
        self.status = status


class TensorDesc(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char_p),
        ("data", ctypes.POINTER(ctypes.c_float)),
        ("ndim", ctypes.c_int32),
        ("shape", ctypes.c_int64 * 4),
    ]


class TraceOp(ctypes.Structure):
    """wsc_trace_op: one entry of Net.trace_plan"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "kind", "in_", "in2", "res", "Ho", "Wo", "C", "coff", "pitch", "kh", "kw", "stride", "pad", "dil", "relu", "affine2", "stride2",
        "pool_rule", "pool_k", "pool_stride", "pool_pad", "pool_avg", "fused_next")] + [("label", ctypes.c_char * 100)]


class TapeEntry(ctypes.Structure):
    """wsc_tape_entry: one kept tensor of Net.seg_tape_plan"""
    _fields_ = [("name", ctypes.c_char * 32), ("Ho", ctypes.c_int32), ("Wo", ctypes.c_int32), ("C", ctypes.c_int32),
                ("offset", ctypes.c_int64)]


class GradEntry(ctypes.Structure):
    """wsc_grad_entry: one layer of SegGrad.layout"""
    _fields_ = [("name", ctypes.c_char * 32), ("kh", ctypes.c_int32), ("kw", ctypes.c_int32), ("Cin", ctypes.c_int32),
                ("Cout", ctypes.c_int32), ("w_off", ctypes.c_int64), ("b_off", ctypes.c_int64)]


TRACE_CONV, TRACE_POOL, TRACE_GATHER, TRACE_HEAD = range(4)
TRACE_INPUT, TRACE_NONE = -1, -2

_lib = None

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_d = ctypes.c_double

# name -> (restype, argtypes); must list every symbol include/wsscam.h declares
_SIGNATURES = {
    "wsc_version": (_i, []),
    "wsc_last_error": (ctypes.c_char_p, []),
    "wsc_ctx_create": (_i, [_i, _vp, ctypes.POINTER(_vp)]),
    "wsc_ctx_destroy": (None, [_vp]),
    "wsc_sync": (_i, [_vp]),
    "wsc_ctx_range_status": (_i, [_vp, ctypes.POINTER(_i), _i]),
    "wsc_ctx_wait": (_i, [_vp, _vp]),
    "wsc_ctx_mark": (_i, [_vp, _i]),
    "wsc_ctx_wait_mark": (_i, [_vp, _i]),
    "wsc_ctx_wait_for_mark": (_i, [_vp, _vp, _i]),
    "wsc_device_info": (_i, [_vp, ctypes.c_char_p, _sz, ctypes.POINTER(_i)]),
    "wsc_malloc": (_i, [_vp, _sz, ctypes.POINTER(_vp)]),
    "wsc_free": (_i, [_vp, _vp]),
    "wsc_memcpy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "wsc_memcpy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "wsc_memset": (_i, [_vp, _vp, _i, _sz]),
    "wsc_ctx_set_option": (_i, [_vp, _i, _i]),
    "wsc_ctx_scratch_fill": (_i, [_vp, _i]),
    "wsc_ctx_scratch_fill_value": (_i, [_vp]),
    "wsc_host_alloc": (_i, [_vp, _sz, ctypes.POINTER(_vp)]),
    "wsc_host_free": (_i, [_vp, _vp]),
    "wsc_host_write_segments": (_i, [ctypes.c_char_p, _i, ctypes.POINTER(_vp), ctypes.POINTER(_sz)]),
    "wsc_memcpy_h2d_async": (_i, [_vp, _vp, _vp, _sz]),
    "wsc_memcpy_d2h_async": (_i, [_vp, _vp, _vp, _sz]),
    "wsc_profile_begin": (_i, [_vp]),
    "wsc_profile_end": (_i, [_vp, _i, _vp, _vp, _vp, ctypes.POINTER(_i)]),
    "wsc_profile_class_name": (ctypes.c_char_p, [_i]),
    "wsc_timer_begin": (_i, [_vp]),
    "wsc_timer_end": (_i, [_vp, ctypes.POINTER(_f)]),
    "wsc_net_create": (_i, [_vp, _i, ctypes.POINTER(TensorDesc), _i, _i, _i, ctypes.POINTER(_vp)]),
    "wsc_net_destroy": (None, [_vp]),
    "wsc_net_cam_size": (_i, [_vp, _i, ctypes.POINTER(_i)]),
    "wsc_net_feat_channels": (_i, [_vp, ctypes.POINTER(_i)]),
    "wsc_net_forward_cam": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "wsc_net_forward_gradcam": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "wsc_net_forward_features": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "wsc_net_cam_size_hw": (_i, [_vp, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "wsc_net_forward_cam_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "wsc_net_forward_edge": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "wsc_net_edge_size": (_i, [_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "wsc_net_forward_edge_raw": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "wsc_irn_aff_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "wsc_cls_loss": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wsc_roc_thresholds": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "wsc_cls_threshold_counts": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "wsc_cls_scores_append": (_i, [_vp, _vp, ctypes.c_longlong, _vp]),
    "wsc_batch_norm_train_nhwc": (_i, [_vp, _vp, ctypes.c_longlong, _i, _vp, _vp, _f, _f, _i, _vp, _vp, _vp]),
    "wsc_batch_norm_grad_nhwc": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _i, _vp, _vp, _vp]),
    "wsc_pool_tf_grad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_maxpool_grad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_net_cls_tape_plan": (_i, [_vp, _vp, _i, _i, _i, ctypes.POINTER(TapeEntry), _i, ctypes.POINTER(_i),
                                   ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_net_forward_cls_train": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, ctypes.c_longlong, _vp]),
    "wsc_cls_grad_create": (_i, [_vp, _vp, ctypes.POINTER(TensorDesc), _i, ctypes.POINTER(_vp)]),
    "wsc_cls_grad_destroy": (None, [_vp]),
    "wsc_cls_grad_layout": (_i, [_vp, ctypes.POINTER(GradEntry), _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_net_backward_cls": (_i, [_vp, _vp, _i, _i, _i, _vp, ctypes.c_longlong, _vp, _vp, ctypes.c_longlong]),
    "wsc_batch_norm_train_drop_nhwc": (_i, [_vp, _vp, ctypes.c_longlong, _i, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _f, ctypes.c_ulonglong,
                                            ctypes.c_longlong, _i]),
    "wsc_batch_norm_grad_drop_nhwc": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _i, _vp, _vp, _vp, _f, ctypes.c_ulonglong,
                                           ctypes.c_longlong, _i]),
    "wsc_net_cls_feat_dims": (_i, [_vp, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "wsc_net_forward_cls_train_drop": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _f,
                                            ctypes.c_ulonglong, ctypes.c_longlong]),
    "wsc_net_backward_cls_drop": (_i, [_vp, _vp, _i, _i, _i, _vp, ctypes.c_longlong, _vp, _vp, ctypes.c_longlong, ctypes.c_longlong, _f,
                                       ctypes.c_ulonglong, ctypes.c_longlong]),
    "wsc_cls_param_layout": (_i, [_vp, ctypes.POINTER(GradEntry), _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_cls_sgd_step": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _f, _f, _i]),
    "wsc_net_cls_load_params": (_i, [_vp, _vp, _vp, _vp, ctypes.c_longlong, _vp]),
    "wsc_cls_train_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _f, _vp, _f, _f, _vp]),
    "wsc_net_edge_tape_plan": (_i, [_vp, _vp, _i, _i, ctypes.POINTER(TapeEntry), _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_net_forward_edge_tape": (_i, [_vp, _vp, _vp, _i, _i, _vp, ctypes.c_longlong, _vp, _vp]),
    "wsc_irn_grad_create": (_i, [_vp, _vp, ctypes.POINTER(TensorDesc), _i, ctypes.POINTER(_vp)]),
    "wsc_irn_grad_destroy": (None, [_vp]),
    "wsc_irn_grad_layout": (_i, [_vp, ctypes.POINTER(GradEntry), _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_net_backward_edge": (_i, [_vp, _vp, _i, _i, _vp, ctypes.c_longlong, _vp, _vp, _vp, ctypes.c_longlong]),
    "wsc_irn_sgd_step": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _f, _f, _f, _f]),
    "wsc_net_irn_load_params": (_i, [_vp, _vp, _vp, _vp, ctypes.c_longlong]),
    "wsc_channel_mean_nchw": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "wsc_net_set_mean_shift": (_i, [_vp, ctypes.POINTER(_f)]),
    "wsc_net_get_mean_shift": (_i, [_vp, ctypes.POINTER(_f)]),
    "wsc_relu_upsample_grad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_group_norm_grad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _vp, _vp]),
    "wsc_rw_propagate": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _i, _vp]),
    "wsc_rw_propagate_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _i, _vp]),
    "wsc_conv2d_nchw": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "wsc_conv2d_nchw_dil": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "wsc_net_seg_size_hw": (_i, [_vp, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "wsc_net_forward_seg": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "wsc_net_seg_tape_plan": (_i, [_vp, _vp, _i, _i, _i, ctypes.POINTER(TapeEntry), _i, ctypes.POINTER(_i),
                                   ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_net_forward_seg_tape": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, ctypes.c_longlong, _vp, _vp]),
    "wsc_net_forward_seg_train": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, ctypes.c_ulonglong, ctypes.c_longlong, _vp, ctypes.c_longlong,
                                       _vp, _vp]),
    "wsc_seg_dropout_f32": (_i, [_vp, _vp, ctypes.c_longlong, ctypes.c_longlong, _f, ctypes.c_ulonglong, ctypes.c_longlong, _i, _vp, _vp]),
    "wsc_net_backward_seg_drop": (_i, [_vp, _vp, _i, _i, _i, _vp, ctypes.c_longlong, _vp, _vp, ctypes.c_longlong, _f]),
    "wsc_relu_bias_grad_scaled": (_i, [_vp, _vp, _vp, ctypes.c_longlong, _i, _f, _vp, _vp]),
    "wsc_seg_grad_create": (_i, [_vp, _vp, ctypes.POINTER(TensorDesc), _i, ctypes.POINTER(_vp)]),
    "wsc_seg_grad_destroy": (None, [_vp]),
    "wsc_seg_grad_layout": (_i, [_vp, ctypes.POINTER(GradEntry), _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong)]),
    "wsc_net_backward_seg": (_i, [_vp, _vp, _i, _i, _i, _vp, ctypes.c_longlong, _vp, _vp, ctypes.c_longlong]),
    "wsc_conv2d_wgrad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "wsc_seg_sgd_accumulate": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _f, _i, _vp]),
    "wsc_seg_sgd_apply": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _f, _f, _i]),
    "wsc_net_seg_load_params": (_i, [_vp, _vp, _vp, _vp, ctypes.c_longlong]),
    "wsc_conv2d_dgrad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_relu_bias_grad": (_i, [_vp, _vp, _vp, ctypes.c_longlong, _i, _vp, _vp]),
    "wsc_pool_same_grad_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_resize_bilinear_tf": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i]),
    "wsc_pool_same_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_pool_tf_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_group_norm_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_maxpool_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "wsc_gap_linear_sigmoid": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    "wsc_cam_flip_add": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "wsc_irn_edge_finish": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    "wsc_fc8_softmax": (_i, [_vp, _vp, _i, ctypes.c_longlong, _i, _f, _vp, _vp]),
    "wsc_net_trace_plan": (_i, [_vp, _vp, _i, _i, _i, ctypes.POINTER(TraceOp), _i, ctypes.POINTER(_i)]),
    "wsc_net_forward_trace": (_i, [_vp, _vp, _vp, _i, _i, _i, ctypes.POINTER(ctypes.c_longlong), _i, _vp, ctypes.c_longlong]),
    "wsc_cam_postprocess": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wsc_cam_eval_confusion": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _vp, _vp]),
    "wsc_unary_from_maps": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "wsc_cam_unary": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "wsc_cam_unary_pm": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "wsc_cam_sum_scales": (_i, [_vp, _vp, _i, _i, ctypes.c_longlong, _vp]),
    "wsc_cam_eval_confusion_nn": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "wsc_label_confusion_nn": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "wsc_render_labels": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "wsc_sem_seg_finish": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp]),
    "wsc_bilinear_resize": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i]),
    "wsc_msf_input_u8": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "wsc_resize_u8": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "wsc_pil_resize_u8": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "wsc_irn_train_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "wsc_label_unary_from_cam": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp]),
    "wsc_ir_label_combine": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "wsc_dsrg_seed_grow": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp]),
    "wsc_seg_loss": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _f, _vp, _f, _vp, _vp, _vp]),
    "wsc_cue_maps": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "wsc_cue_seeds": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _i, _d, _vp, _vp]),
    "wsc_seg_unary_nhwc": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "wsc_seg_resize_argmax": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "wsc_seg_preprocess_u8": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "wsc_seg_crf_image_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    "wsc_seg_crf_logprob": (_i, [_vp, _vp, _i, _i, ctypes.c_longlong, _f, _vp]),
    "wsc_seg_planes_from_nhwc": (_i, [_vp, _vp, _i, _i, ctypes.c_longlong, _vp]),
    "wsc_seg_train_batch": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "wsc_seg_gt_index_tf": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    "wsc_hsn_gradcam_post": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _i]),
    "wsc_hsn_voc_background": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "wsc_hsn_class_mass": (_i, [_vp, _vp, _i, _i, _vp]),
    "wsc_hsn_background": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "wsc_cam_adp_modify": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp]),
    "wsc_hsn_cs_gradcam": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "wsc_hsn_gather_unary": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "wsc_crf_create": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _f, ctypes.POINTER(_vp)]),
    "wsc_crf_destroy": (None, [_vp]),
    "wsc_crf_lattice_sizes": (_i, [_vp, _vp, _vp, _vp]),
    "wsc_crf_gaussian_on_chip": (_i, [_vp, _i]),
    "wsc_crf_inference": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp]),
    "wsc_crf_inference_pm": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp]),
    "wsc_crf_v_create": (_i, [_vp, _vp, _vp, _i, _f, _f, _f, ctypes.POINTER(_vp)]),
    "wsc_crf_v_destroy": (None, [_vp]),
    "wsc_crf_v_num_groups": (_i, [_vp]),
    "wsc_crf_v_inference": (_i, [_vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp]),
}


def header_symbols():
    """Function names declared in include/wsscam.h."""
    with open(HEADER_PATH) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wsc_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load libwsscam.so (no GPU needed for loading; compute calls need one)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WscError(WSC_ERR_NO_DEVICE,
                       "libwsscam.so not built at %s -- run `python __graft_entry__.py` (there is no "
                       "CPU fallback for the product path)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check_exports():
    """Every symbol the header declares must be exported and bound."""
    lib = load()
    declared = header_symbols()
    missing = [s for s in declared if not hasattr(lib, s)]
    unbound = [s for s in declared if s not in _SIGNATURES]
    if missing or unbound:
        raise WscError(WSC_ERR_INVALID, "missing exports %s / unbound %s" % (missing, unbound))
    return declared


def check(status):
    if status != WSC_OK:
        raise WscError(status, load().wsc_last_error().decode("utf-8", "replace"))


def _ptr(x):
    """Device pointer of a DeviceBuffer / torch tensor / int, or host pointer of a numpy array."""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):  # torch tensor
        return x.data_ptr()
    raise TypeError("cannot take a pointer of %r" % type(x))


def _two_call(fn, args, entry_type, extra=0):
    """The "count, allocate, fill" idiom of every plan / layout entry point: fn(*args, None, 0, &n, &extra...) for the count, then
    the same call with room for n entries of `entry_type` -> (the entries, the `extra` trailing long long out-parameters)."""
    n, tail = _i(), [ctypes.c_longlong() for _ in range(extra)]
    refs = [ctypes.byref(v) for v in [n] + tail]
    check(fn(*args, None, 0, *refs))
    ent = (entry_type * n.value)()
    check(fn(*args, ent, n.value, *refs))
    return ent, [v.value for v in tail]


def _tape_plan(fn, *args):
    """a wsc_net_*_tape_plan entry point -> ([{'name', 'Ho', 'Wo', 'C', 'offset'}], tape_elems)"""
    ent, (elems,) = _two_call(fn, args, TapeEntry, 1)
    return [{"name": e.name.decode(), "Ho": e.Ho, "Wo": e.Wo, "C": e.C, "offset": e.offset} for e in ent], elems


class StackChain:
    """One GPU-filling phase at a time across the contexts of a driver's lanes.  `run(ctx, enqueue)` makes what `enqueue()` puts
    on ctx's stream wait -- on the device, wsc_ctx_wait_for_mark -- for the phase the chain ran last on another context.  A conv
    stack fills the GPU by itself: two of them interleaved by the hardware scheduler ran 8.5 ms each = 7.1 ms per batch where
    back to back they take 6.3 (step.make_cam through step.pipeline, round 6: 4490 -> 5110 images/s); the other lanes' uploads,
    tails, CRFs and read-backs still overlap the running stack.  Marker slot 7 of the lanes' contexts belongs to the chain."""

    SLOT = 7

    def __init__(self):
        self._lock = threading.Lock()
        self._last = None

    def run(self, ctx, enqueue):
        with self._lock:
            prev = self._last
            if prev is not None and prev is not ctx:
                ctx.wait_for_mark(prev, self.SLOT)
            try:
                return enqueue()
            finally:
                ctx.mark(self.SLOT)
                self._last = ctx


class Context:
    """wsc_ctx: one device + one stream (make_cam.py:31-33 `cuda.device(process_id)`)."""

    def __init__(self, device=0, stream=None):
        lib = load()
        h = _vp()
        check(lib.wsc_ctx_create(int(device), stream, ctypes.byref(h)))
        self.h = h
        self.device = device
        self._lib = lib
        self._options = {}  # selectors set through set_option (the library has no getter; option() restores from here)

    def close(self):
        if getattr(self, "h", None):
            pool = self.__dict__.pop("_pool", None)
            if pool:
                for lst in pool.values():
                    for buf in lst:
                        self._lib.wsc_free(self.h, buf.ptr)
                        buf.ptr = None
            self._lib.wsc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.wsc_sync(self.h))

    def drain(self):
        """sync() for the release paths: waits for the stream, and leaves a raised range flag to the next sync() / to_host()
        instead of raising WSC_ERR_RANGE itself (the flag is sticky, so nothing is lost; what has to be freed is freed)."""
        st = self._lib.wsc_sync(self.h)
        if st != WSC_ERR_RANGE:
            check(st)

    def range_status(self, clear=False):
        """Range guard of the IEEE-half conv modes: 0 = clean, else the output-channel count of a layer whose activations
        reached half's ceiling and were saturated (sync() / to_host() raise WscError(WSC_ERR_RANGE) until cleared)."""
        f = _i(0)
        check(self._lib.wsc_ctx_range_status(self.h, ctypes.byref(f), 1 if clear else 0))
        return int(f.value)

    def mark(self, slot):
        """Records marker `slot` (0 .. 7) at the current end of this context's stream (wsc_ctx_mark)."""
        check(self._lib.wsc_ctx_mark(self.h, int(slot)))

    def wait_mark(self, slot):
        """Host wait for everything enqueued before the marker's last record (returns at once if never recorded)."""
        check(self._lib.wsc_ctx_wait_mark(self.h, int(slot)))

    def wait_for_mark(self, other, slot):
        """Device-side join with marker `slot` of `other`: later work on this ctx waits for what `other` had enqueued when it
        last recorded the marker -- not for anything it enqueued afterwards."""
        check(self._lib.wsc_ctx_wait_for_mark(self.h, other.h, int(slot)))

    def wait_for(self, other):
        """Device-side join: later work on this ctx waits for everything enqueued so far on `other`."""
        check(self._lib.wsc_ctx_wait(self.h, other.h))

    def device_info(self):
        buf = ctypes.create_string_buffer(128)
        n = _i()
        check(self._lib.wsc_device_info(self.h, buf, 128, ctypes.byref(n)))
        return buf.value.decode(), n.value

    def alloc(self, nbytes, pooled=False):
        """pooled=True: the block comes from / returns to a per-context free list instead of hipMalloc / hipFree (both
        synchronise the device).  Only for buffers that are used on THIS context's stream alone: reuse is ordered by
        the stream, exactly like the library's internal cached allocator."""
        nbytes = int(nbytes)
        if pooled:
            size = 1 << max(16, (max(nbytes, 1) - 1).bit_length())
            pool = self.__dict__.setdefault("_pool", {})
            lst = pool.get(size)
            if lst:
                buf = lst.pop()
                buf.nbytes = nbytes
                return buf
            buf = DeviceBuffer(self, size)
            buf.nbytes, buf._pool_size = nbytes, size
            return buf
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr, pooled=False):
        arr = np.ascontiguousarray(arr)
        buf = self.alloc(arr.nbytes, pooled=pooled)
        try:
            check(self._lib.wsc_memcpy_h2d(self.h, buf.ptr, arr.ctypes.data, arr.nbytes))
            self.drain()  # arr may be a temporary; an earlier call's range error is not this copy's to report
        except Exception:
            buf.free()
            raise
        return buf

    def to_host(self, buf, shape, dtype, offset_bytes=0):
        out = np.empty(shape, dtype=dtype)
        check(self._lib.wsc_memcpy_d2h(self.h, out.ctypes.data, _ptr(buf) + offset_bytes, out.nbytes))
        return out

    def host_alloc(self, nbytes):
        """Page-locked host buffer (wsc_host_alloc) for asynchronous copies."""
        return PinnedBuffer(self, int(nbytes))

    def h2d_async(self, dst_dev, pinned, nbytes, dst_offset=0, src_offset=0):
        check(self._lib.wsc_memcpy_h2d_async(self.h, _ptr(dst_dev) + dst_offset, pinned.ptr + src_offset, int(nbytes)))

    def d2h_async(self, pinned, src_dev, nbytes, dst_offset=0, src_offset=0):
        check(self._lib.wsc_memcpy_d2h_async(self.h, pinned.ptr + dst_offset, _ptr(src_dev) + src_offset, int(nbytes)))

    def set_option(self, option, value):
        """A path selector of this context (OPT_*): forces a fallback path that gives the same bits (testing / debugging) --
        except OPT_CAM_HEAD_STREAM, whose two paths sum K in different orders and agree to fp32 round-off (2e-6 relative) only."""
        check(self._lib.wsc_ctx_set_option(self.h, int(option), int(value)))
        self._options[int(option)] = int(value)

    def get_option(self, option):
        """The selector's current value (what set_option last stored; OPT_DEFAULTS before that)."""
        return self._options.get(int(option), OPT_DEFAULTS[int(option)])

    def option(self, option, value):
        """Context manager: the selector is set inside the block and back to the value it HAD afterwards (an earlier
        set_option or an enclosing option() block stays in force)."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            before = self.get_option(option)
            self.set_option(option, value)
            try:
                yield self
            finally:
                self.set_option(option, before)

        return _cm()

    def scratch_fill(self, value):
        """Context manager (testing): inside the block the workspace arena and every cached scratch block this context hands to
        a kernel hold the byte `value` (0 .. 255) instead of what the previous call left; the fill is off again afterwards,
        whatever happened inside.  Results must not depend on it (wsc_ctx_scratch_fill)."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            check(self._lib.wsc_ctx_scratch_fill(self.h, int(value)))
            try:
                yield self
            finally:
                check(self._lib.wsc_ctx_scratch_fill(self.h, -1))

        return _cm()

    def scratch_fill_value(self):
        """-1 (off) or the byte of the scratch fill that is on (wsc_ctx_scratch_fill_value)."""
        return int(self._lib.wsc_ctx_scratch_fill_value(self.h))

    def profile_begin(self):
        check(self._lib.wsc_profile_begin(self.h))

    def profile_end(self):
        """-> {class name: (launches, total_ms, algorithmic work)} for the launches since profile_begin."""
        n = 16
        calls = np.zeros(n, np.int32)
        ms = np.zeros(n, np.float32)
        work = np.zeros(n, np.float64)
        k = _i()
        check(self._lib.wsc_profile_end(self.h, n, calls.ctypes.data, ms.ctypes.data, work.ctypes.data, ctypes.byref(k)))
        return {self._lib.wsc_profile_class_name(i).decode(): (int(calls[i]), float(ms[i]), float(work[i]))
                for i in range(k.value) if calls[i] > 0}

    def timer_begin(self):
        check(self._lib.wsc_timer_begin(self.h))

    def timer_end(self):
        ms = _f()
        check(self._lib.wsc_timer_end(self.h, ctypes.byref(ms)))
        return ms.value


class DeviceBuffer:
    """hipMalloc'ed bytes owned through wsc_malloc / wsc_free."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = nbytes
        p = _vp()
        check(ctx._lib.wsc_malloc(ctx.h, nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def free(self):
        if getattr(self, "ptr", None) and self.ctx.h:
            size = getattr(self, "_pool_size", None)
            if size is not None and getattr(self.ctx, "_pool", None) is not None:
                twin = DeviceBuffer.__new__(DeviceBuffer)  # the block lives on in the pool under a fresh handle
                twin.ctx, twin.nbytes, twin.ptr, twin._pool_size = self.ctx, size, self.ptr, size
                self.ctx._pool.setdefault(size, []).append(twin)
                self.ptr = None
                return
            self.ctx._lib.wsc_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedBuffer:
    """hipHostMalloc'ed bytes; `.view(shape, dtype, offset)` is a numpy array over them (no copy)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = nbytes
        p = _vp()
        check(ctx._lib.wsc_host_alloc(ctx.h, nbytes, ctypes.byref(p)))
        self.ptr = p.value
        self._raw = (ctypes.c_char * max(nbytes, 1)).from_address(self.ptr)

    def view(self, shape, dtype, offset_bytes=0):
        n = int(np.prod(shape)) if len(shape) else 1
        return np.frombuffer(self._raw, dtype=dtype, count=n, offset=offset_bytes).reshape(shape)

    def free(self):
        if getattr(self, "ptr", None) and self.ctx.h:
            self._raw = None
            self.ctx._lib.wsc_host_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def host_write_segments(path, segments):
    """wsc_host_write_segments: `segments` = bytes objects / C-contiguous numpy arrays, written to `path` one after the other by
    one C call (open + writev + close) -- the interpreter lock is released for its whole duration."""
    n = len(segments)
    ptrs = (_vp * max(n, 1))()
    sizes = (_sz * max(n, 1))()
    keep = []
    for i, sgm in enumerate(segments):
        if isinstance(sgm, np.ndarray):
            assert sgm.flags["C_CONTIGUOUS"]
            ptrs[i], sizes[i] = sgm.ctypes.data, sgm.nbytes
        else:
            sgm = bytes(sgm)
            keep.append(sgm)  # (the pointer below is the bytes object's own buffer)
            ptrs[i], sizes[i] = ctypes.cast(ctypes.c_char_p(sgm), _vp).value, len(sgm)
    check(load().wsc_host_write_segments(os.fsencode(path), n, ptrs, sizes))


def make_tensor_descs(state_dict):
    """dict name -> numpy float32 array  ->  (ctypes array of TensorDesc, keep-alive list)."""
    keep = []
    items = []
    for name, arr in state_dict.items():
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        if a.ndim > 4:
            continue
        keep.append(a)
        d = TensorDesc()
        d.name = name.encode()
        d.data = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        d.ndim = a.ndim
        for k in range(4):
            d.shape[k] = a.shape[k] if k < a.ndim else 1
        items.append(d)
    arr_t = TensorDesc * len(items)
    return arr_t(*items), keep


class Net:
    """wsc_net: packed weights of one CAM network."""

    def __init__(self, ctx, arch, state_dict, num_classes, precision=PREC_F16X3):
        self.ctx = ctx
        self.arch = arch
        self.num_classes = num_classes
        self.precision = precision
        descs, keep = make_tensor_descs(state_dict)
        h = _vp()
        check(ctx._lib.wsc_net_create(ctx.h, arch, descs, len(descs), num_classes, precision, ctypes.byref(h)))
        del keep
        self.h = h

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            try:
                self.ctx.drain()
            finally:  # (whatever the wait reports, the weights are released)
                h, self.h = self.h, None
                self.ctx._lib.wsc_net_destroy(h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cam_size(self, S):
        n = _i()
        check(self.ctx._lib.wsc_net_cam_size(self.h, S, ctypes.byref(n)))
        return n.value

    def feat_channels(self):
        n = _i()
        check(self.ctx._lib.wsc_net_feat_channels(self.h, ctypes.byref(n)))
        return n.value

    def forward_cam(self, x_dev, B, S, cam_dev, score_dev=None, ctx=None):
        """ctx: the context (stream, activation arena) to run on; the packed weights are read-only and shared."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_cam(run.h, self.h, _ptr(x_dev), B, S, _ptr(cam_dev),
                                                _ptr(score_dev)))

    def cam_size_hw(self, H, W):
        h, w = _i(), _i()
        check(self.ctx._lib.wsc_net_cam_size_hw(self.h, int(H), int(W), ctypes.byref(h), ctypes.byref(w)))
        return h.value, w.value

    def forward_cam_hw(self, x_dev, B, H, W, cam_dev, score_dev=None, ctx=None):
        """Non-square network input [B][2][3][H][W] (outsize = None: the image's own size)."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_cam_hw(run.h, self.h, _ptr(x_dev), B, int(H), int(W), _ptr(cam_dev), _ptr(score_dev)))

    def forward_gradcam(self, x_dev, N, S, relu, cams_dev, score_dev=None, ctx=None):
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_gradcam(run.h, self.h, _ptr(x_dev), N, S, int(relu), _ptr(cams_dev),
                                                    _ptr(score_dev)))

    def forward_features(self, x_dev, N, S, feat_dev):
        check(self.ctx._lib.wsc_net_forward_features(self.ctx.h, self.h, _ptr(x_dev), N, S, _ptr(feat_dev)))

    def forward_edge(self, x_dev, B, S, feat_h, feat_w, edge_dev, dp_dev, ctx=None):
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_edge(run.h, self.h, _ptr(x_dev), B, S, feat_h, feat_w,
                                                 _ptr(edge_dev), _ptr(dp_dev)))

    def edge_size(self, S):
        """((He, We), (Hd, Wd)): the sizes of edge_out and dp_out of an ARCH_*_IRN net for an S x S input."""
        e, d = (_i * 2)(), (_i * 2)()
        check(self.ctx._lib.wsc_net_edge_size(self.h, int(S), e, d))
        return (e[0], e[1]), (d[0], d[1])

    def forward_edge_raw(self, x_dev, N, S, edge_dev, dp_dev, ctx=None):
        """Net.forward in training mode (wsc_net_forward_edge_raw): x_dev [N][3][S][S] -> edge_out [N][He][We], dp_out [N][2][Hd][Wd]."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_edge_raw(run.h, self.h, _ptr(x_dev), int(N), int(S), _ptr(edge_dev), _ptr(dp_dev)))

    def set_mean_shift(self, m):
        """wsc_net_set_mean_shift: the two floats (mean_shift.running_mean) forward_edge subtracts from dp."""
        check(self.ctx._lib.wsc_net_set_mean_shift(self.h, (_f * 2)(float(m[0]), float(m[1]))))

    def get_mean_shift(self):
        m = (_f * 2)()
        check(self.ctx._lib.wsc_net_get_mean_shift(self.h, m))
        return np.array([m[0], m[1]], np.float32)

    def edge_tape_plan(self, N, S):
        """wsc_net_edge_tape_plan: ([{'name', 'Ho', 'Wo', 'C', 'offset'}], tape_elems) -- what the backward pass of the heads needs
        of a forward pass of N samples of S x S: "x<k>" stage taps, "<head>.z", "<head>.stats" ([N][1][1][2 G] {mean, rstd}
        pairs), "cat<i>" concat buffers, float32 at `offset` floats of one buffer of tape_elems floats."""
        return _tape_plan(self.ctx._lib.wsc_net_edge_tape_plan, self.ctx.h, self.h, int(N), int(S))

    def forward_edge_tape(self, x_dev, N, S, tape_dev, tape_elems, edge_dev, dp_dev, ctx=None):
        """wsc_net_forward_edge_tape: forward_edge_raw (the same bits) that also fills tape_dev (float32, tape_elems of them)."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_edge_tape(run.h, self.h, _ptr(x_dev), int(N), int(S), _ptr(tape_dev), int(tape_elems),
                                                      _ptr(edge_dev), _ptr(dp_dev)))

    def backward_edge(self, grad, N, S, tape_dev, tape_elems, dedge_dev, ddp_dev, grad_dev, grad_elems=None, ctx=None):
        """wsc_net_backward_edge through `grad`, the IrnGrad of this net: dedge_dev [N][He][We], ddp_dev [N][2][Hd][Wd] -> every
        element of grad_dev (grad.grad_elems floats in grad.layout)."""
        if grad.net is not self:
            raise ValueError("backward_edge: the IrnGrad was created for another net")
        grad.backward(N, S, tape_dev, tape_elems, dedge_dev, ddp_dev, grad_dev, grad_elems=grad_elems, ctx=ctx)

    def seg_size_hw(self, H, W):
        """The fc8 map size of an ARCH_DEEPLAB_* net for an H x W input (41 x 41 at 321 x 321)."""
        h, w = _i(), _i()
        check(self.ctx._lib.wsc_net_seg_size_hw(self.h, int(H), int(W), ctypes.byref(h), ctypes.byref(w)))
        return h.value, w.value

    def forward_seg(self, x_dev, B, H, W, prob_dev, fc8_dev=None, min_prob=1e-4, ctx=None):
        """SEC / DSRG forward pass (wsc_net_forward_seg): x_dev float32 [B][H][W][3] NHWC (BGR minus mean) ->
        prob_dev float32 [B][h][w][C] fc8-softmax, fc8_dev (optional) the logits in the same layout."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_seg(run.h, self.h, _ptr(x_dev), int(B), int(H), int(W), float(min_prob), _ptr(fc8_dev),
                                                _ptr(prob_dev)))

    def seg_tape_plan(self, B, H, W):
        """wsc_net_seg_tape_plan: ([{'name', 'Ho', 'Wo', 'C', 'offset'}], tape_elems) -- the tensors a backward pass needs of a
        forward pass of a B x H x W input, float32 NHWC at `offset` floats of one buffer of tape_elems floats."""
        return _tape_plan(self.ctx._lib.wsc_net_seg_tape_plan, self.ctx.h, self.h, int(B), int(H), int(W))

    def forward_seg_tape(self, x_dev, B, H, W, tape_dev, tape_elems, prob_dev, fc8_dev=None, min_prob=1e-4, ctx=None):
        """wsc_net_forward_seg_tape: forward_seg with the tape's tensors copied to tape_dev (float32, tape_elems of them)."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_seg_tape(run.h, self.h, _ptr(x_dev), int(B), int(H), int(W), float(min_prob), _ptr(tape_dev),
                                                     int(tape_elems), _ptr(fc8_dev), _ptr(prob_dev)))

    def forward_seg_train(self, x_dev, B, H, W, drop_prob, seed, step, tape_dev, tape_elems, prob_dev, fc8_dev=None, min_prob=1e-4, ctx=None):
        """wsc_net_forward_seg_train: forward_seg_tape with the dropout sites behind fc6 / fc7 active -- keep-masks of
        (seed, step, site, element index), the tape's fc6* / fc7* entries the dropped, scaled activations."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_seg_train(run.h, self.h, _ptr(x_dev), int(B), int(H), int(W), float(min_prob), float(drop_prob),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), _ptr(tape_dev), int(tape_elems),
                                                      _ptr(fc8_dev), _ptr(prob_dev)))

    def cls_tape_plan(self, B, H, W):
        """wsc_net_cls_tape_plan: ([{'name', 'Ho', 'Wo', 'C', 'offset'}], tape_elems) -- what the backward pass of an
        ARCH_VGG16_CAM / ARCH_M7_CAM net needs of a training forward pass of a B x H x W input: "input", per conv "<key>" (post-ReLU),
        on BatchNorm nets "<key>.bn" and "<key>.stats" ([1][1][1][2 C] {mean, rstd} pairs), "pool:<i>"."""
        return _tape_plan(self.ctx._lib.wsc_net_cls_tape_plan, self.ctx.h, self.h, int(B), int(H), int(W))

    def forward_cls_train(self, x_dev, B, H, W, tape_dev, tape_elems, feat_dev, keep=0.99, unbiased=True, run_dev=None, ctx=None):
        """wsc_net_forward_cls_train: x_dev [B][3][H][W] -> the tape and feat_dev [B][h][w][F]; BatchNorm on the batch statistics;
        run_dev (optional): every BatchNorm layer's [2][C] running mean / variance in stack order, updated in place with `keep`
        the weight of the OLD value (Keras' momentum)."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_cls_train(run.h, self.h, _ptr(x_dev), int(B), int(H), int(W), float(keep), int(bool(unbiased)),
                                                      _ptr(run_dev), _ptr(tape_dev), int(tape_elems), _ptr(feat_dev)))

    def cls_feat_dims(self, H, W, dropping=False):
        """wsc_net_cls_feat_dims: (h, w) of the map forward_cls_train[_drop] writes and ClsLoss reduces for an H x W input; with
        `dropping` (drop_prob > 0) an M7 net's is the pooled, dropped layer3_p2 map."""
        h, w = _i(), _i()
        check(self.ctx._lib.wsc_net_cls_feat_dims(self.h, int(H), int(W), int(bool(dropping)), ctypes.byref(h), ctypes.byref(w)))
        return h.value, w.value

    def forward_cls_train_drop(self, x_dev, B, H, W, tape_dev, tape_elems, feat_dev, feat_elems, drop_prob, seed, step, keep=0.99,
                               unbiased=True, run_dev=None, ctx=None):
        """wsc_net_forward_cls_train_drop: forward_cls_train with the dropout sites active -- keep-masks of (seed, step, site,
        element index); feat_dev holds feat_elems = B h w F floats, (h, w) = cls_feat_dims(H, W, drop_prob > 0).  At drop_prob = 0
        the launches and bits of forward_cls_train."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_forward_cls_train_drop(run.h, self.h, _ptr(x_dev), int(B), int(H), int(W), float(keep), int(bool(unbiased)),
                                                           _ptr(run_dev), _ptr(tape_dev), int(tape_elems), _ptr(feat_dev), int(feat_elems),
                                                           float(drop_prob), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)))

    def trace_plan(self, N, H, W, ctx=None):
        """wsc_net_trace_plan: one dict per op of the stack for an N x H x W input (+ the CAM head), the fields of wsc_trace_op
        (`in` under its own name, the label as str).  Follows the options of `ctx` (the fused stem)."""
        run = ctx or self.ctx
        ops, _ = _two_call(self.ctx._lib.wsc_net_trace_plan, (run.h, self.h, int(N), int(H), int(W)), TraceOp)
        out = []
        for o in ops:
            d = {name.rstrip("_"): getattr(o, name) for name, _ in TraceOp._fields_ if name != "label"}
            d["label"] = o.label.decode()
            out.append(d)
        return out

    def forward_trace(self, x_dev, N, H, W, offsets, trace_dev, trace_elems, ctx=None):
        """wsc_net_forward_trace: entry i of the plan as float32 [N][Ho][Wo][pitch] at trace_dev + offsets[i] floats (< 0: skipped)."""
        run = ctx or self.ctx
        off = (ctypes.c_longlong * len(offsets))(*[int(o) for o in offsets])
        check(self.ctx._lib.wsc_net_forward_trace(run.h, self.h, _ptr(x_dev), int(N), int(H), int(W), off, len(offsets), _ptr(trace_dev),
                                                  int(trace_elems)))


# ---- the parameter codec: {name: tensor} <-> one flat float32 buffer in a gradient layout.  Layouts and arrays in, nothing else: no
# device, no library.  Every flat_params / to_state_dict / to_host / params_host of the training modules is a call into these two.
# Field: one tensor of a flat buffer -- `key` its name (a tuple is a path into nested dicts: ('conv1_1', 'w')), `offset` and `size` in
# floats, `shape` as the caller sees it, `perm` the axis permutation into the stored order (None: it lies as it is), `head`: a tensor
# of more rows than shape[0] gives its first shape[0] (a Linear of more rows than the net has classes).
Field = collections.namedtuple("Field", "key offset size shape perm head", defaults=(None, False))


def flatten(tensors, fields, elems=None):
    """tensors by the fields' keys (arrays or torch tensors; other keys are ignored) -> one float32 array of `elems` floats (None:
    up to the last field's end), every field's tensor in its stored order at its offset.  A missing tensor or a shape that is not
    the field's is a ValueError that names it."""
    flat = np.empty((max([f.offset + f.size for f in fields] + [0]) if elems is None else int(elems),), np.float32)
    for f in fields:
        v = tensors
        for k in f.key if isinstance(f.key, tuple) else (f.key,):
            if not hasattr(v, "keys") or k not in v:
                raise ValueError("flatten: there is no tensor %r" % (f.key,))
            v = v[k]
        v = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
        if f.head and v.ndim == len(f.shape) and v.shape[0] >= f.shape[0]:
            v = v[:f.shape[0]]
        if tuple(v.shape) != tuple(f.shape):
            raise ValueError("flatten: %r is %r, the layout has %r" % (f.key, tuple(v.shape), tuple(f.shape)))
        flat[f.offset:f.offset + f.size] = (v if f.perm is None else v.transpose(f.perm)).reshape(-1)
    return flat


def unflatten(flat, fields):
    """The inverse of flatten: -> {key: a new array of the field's shape} (a tuple key nests: {'conv1_1': {'w': ...}})."""
    out = {}
    for f in fields:
        v = flat[f.offset:f.offset + f.size]
        if f.perm is None:
            v = v.reshape(f.shape).copy()
        else:
            v = np.ascontiguousarray(v.reshape([f.shape[a] for a in f.perm]).transpose([int(a) for a in np.argsort(f.perm)]))
        path, d = f.key if isinstance(f.key, tuple) else (f.key,), out
        for k in path[:-1]:
            d = d.setdefault(k, {})
        d[path[-1]] = v
    return out


def _named_fields(layout, perm):
    """the fields of an irn / cls layout ([{'name', 'shape', 'offset', 'size', 'conv'}]): conv weights stored under `perm`"""
    return [Field(e["name"], e["offset"], e["size"], tuple(e["shape"]), perm if e["conv"] else None, ".classifier." in e["name"])
            for e in layout]


class _Grad:
    """The handle of a wsc_<KIND>_grad: created from the net and the state dict the net was created from, `grad_elems` and the
    entries of wsc_<KIND>_grad_layout (a subclass shapes them into its `layout`, and fields(layout) says how a layout's tensors
    lie for the codec above), close() / __del__.  The net must outlive it."""
    KIND = None  # "seg" / "irn" / "cls"

    def __init__(self, net, state_dict):
        self.ctx = net.ctx
        self.net = net
        lib = self.ctx._lib
        descs, keep = make_tensor_descs(state_dict)
        h = _vp()
        check(getattr(lib, "wsc_%s_grad_create" % self.KIND)(self.ctx.h, net.h, descs, len(descs), ctypes.byref(h)))
        del keep
        self.h = h
        ent, (self.grad_elems,) = _two_call(getattr(lib, "wsc_%s_grad_layout" % self.KIND), (h,), GradEntry, 1)
        self.layout = self._shape_layout(ent)

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            getattr(self.ctx._lib, "wsc_%s_grad_destroy" % self.KIND)(self.h)  # (drains the stream)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _elems(self, elems):
        return int(self.grad_elems if elems is None else elems)


class SegGrad(_Grad):
    """wsc_seg_grad: what the backward pass of one ARCH_DEEPLAB_* net keeps (the data-gradient kernels, the workspace).
    state_dict: the one the net was created from.  The net must outlive it."""
    KIND = "seg"

    @staticmethod
    def _shape_layout(ent):
        # layer -> its kernel, channels and the float offsets of dW (HWIO) and db in the gradient buffer
        return {e.name.decode(): {"k": e.kh, "Cin": e.Cin, "Cout": e.Cout, "w_off": e.w_off, "b_off": e.b_off} for e in ent}

    @staticmethod
    def fields(layout):
        """per layer (layer, 'w'), HWIO as it lies, and (layer, 'b')"""
        out = []
        for layer, e in layout.items():
            shape = (e["k"], e["k"], e["Cin"], e["Cout"])
            out += [Field((layer, "w"), e["w_off"], e["k"] * e["k"] * e["Cin"] * e["Cout"], shape), Field((layer, "b"), e["b_off"], e["Cout"], (e["Cout"],))]
        return out

    def backward(self, B, H, W, tape_dev, tape_elems, dfc8_dev, grad_dev, grad_elems=None):
        """wsc_net_backward_seg: dfc8_dev float32 [B][h][w][C] -> every element of grad_dev (self.grad_elems floats), on the
        net's own context (the workspace belongs to its stream)."""
        check(self.ctx._lib.wsc_net_backward_seg(self.ctx.h, self.h, int(B), int(H), int(W), _ptr(tape_dev), int(tape_elems), _ptr(dfc8_dev),
                                                 _ptr(grad_dev), self._elems(grad_elems)))

    def backward_drop(self, B, H, W, tape_dev, tape_elems, dfc8_dev, grad_dev, drop_prob, grad_elems=None):
        """wsc_net_backward_seg_drop: backward() on a tape of forward_seg_train at `drop_prob`."""
        check(self.ctx._lib.wsc_net_backward_seg_drop(self.ctx.h, self.h, int(B), int(H), int(W), _ptr(tape_dev), int(tape_elems),
                                                      _ptr(dfc8_dev), _ptr(grad_dev),
                                                      self._elems(grad_elems), float(drop_prob)))

    def sgd_accumulate(self, param_dev, grad_dev, accum_dev, weight_decay, accum_num, l2_dev=None, elems=None, ctx=None):
        """wsc_seg_sgd_accumulate on three buffers of self.grad_elems floats in self.layout: accum += mult (grad [+ weight_decay
        param on weights]) / accum_num; l2_dev (optional, one float) receives loss["l2"]."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_seg_sgd_accumulate(run.h, self.h, _ptr(param_dev), _ptr(grad_dev), _ptr(accum_dev),
                                                   self._elems(elems), float(weight_decay), int(accum_num),
                                                   _ptr(l2_dev)))

    def sgd_apply(self, param_dev, accum_dev, mom_dev, lr, momentum, clear_accum=True, elems=None, ctx=None):
        """wsc_seg_sgd_apply: mom = mom momentum + accum, param -= lr mom, and (clear_accum) accum = 0."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_seg_sgd_apply(run.h, self.h, _ptr(param_dev), _ptr(accum_dev), _ptr(mom_dev),
                                              self._elems(elems), float(lr), float(momentum), int(bool(clear_accum))))

    def load_params(self, param_dev, elems=None, net=None, ctx=None):
        """wsc_net_seg_load_params: the net's packed weights and this object's data-gradient kernels rewritten on the device from
        the flat parameter buffer.  The net must not be in use on another stream."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_seg_load_params(run.h, (net or self.net).h, self.h, _ptr(param_dev),
                                                    self._elems(elems)))


class IrnGrad(_Grad):
    """wsc_irn_grad: what the backward pass of the heads of one ARCH_*_IRN net keeps (the data-gradient kernels, the workspace).
    state_dict: the one the net was created from.  The net must outlive it.
    layout: [{'name', 'shape', 'offset', 'size', 'conv'}] one per parameter in the order of trainable_parameters(), `shape`
    torch's ((Cout, Cin, 1, 1) or (C,)); a conv weight lies as [Cin][Cout] at its offset."""
    KIND = "irn"

    @staticmethod
    def _shape_layout(ent):
        layout = []
        for e in ent:
            conv = e.kh == 1
            layout.append({"name": e.name.decode(), "conv": conv, "shape": (e.Cout, e.Cin, 1, 1) if conv else (e.Cout,),
                           "offset": e.w_off if conv else e.b_off, "size": e.Cin * e.Cout if conv else e.Cout})
        return layout

    def backward(self, N, S, tape_dev, tape_elems, dedge_dev, ddp_dev, grad_dev, grad_elems=None, ctx=None):
        """wsc_net_backward_edge on the net's own context (the workspace belongs to its stream; `ctx`: another one is an error)."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_backward_edge(run.h, self.h, int(N), int(S), _ptr(tape_dev), int(tape_elems), _ptr(dedge_dev),
                                                  _ptr(ddp_dev), _ptr(grad_dev), self._elems(grad_elems)))

    @staticmethod
    def fields(layout):
        """torch's OIHW 1 x 1 weights stored as [Cin][Cout], the vectors as they lie"""
        return _named_fields(layout, (1, 0, 2, 3))

    def flat_params(self, state_dict):
        """The head tensors of a state dict ({name: array in torch's shape}; other keys are ignored) -> one float32 array of
        grad_elems floats in `layout`: the host form of what sgd_step and load_params take (IrnGrads.to_state_dict's inverse)."""
        return flatten(state_dict, self.fields(self.layout), self.grad_elems)

    def sgd_step(self, param_dev, grad_dev, mom_dev, lr_edge, lr_dp, weight_decay, sgd_momentum, elems=None, ctx=None):
        """wsc_irn_sgd_step on three buffers of grad_elems floats in `layout`: g = grad + weight_decay p; m = sgd_momentum m + g;
        p -= lr m with lr_edge on the `fc_edge*` entries and lr_dp on the rest, every product and sum one fp32 rounding."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_irn_sgd_step(run.h, self.h, _ptr(param_dev), _ptr(grad_dev), _ptr(mom_dev),
                                             self._elems(elems), float(lr_edge), float(lr_dp),
                                             float(weight_decay), float(sgd_momentum)))

    def load_params(self, param_dev, elems=None, net=None, ctx=None):
        """wsc_net_irn_load_params: the heads' packed weights and GroupNorm vectors, the two final convs and this object's
        data-gradient kernels rewritten on the device from the flat parameter buffer.  The net must not be in use on another
        stream."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_irn_load_params(run.h, (net or self.net).h, self.h, _ptr(param_dev),
                                                    self._elems(elems)))


class ClsGrad(_Grad):
    """wsc_cls_grad: what the backward pass of one ARCH_VGG16_CAM / ARCH_M7_CAM net keeps (the data-gradient kernels, the
    workspace).  state_dict: the one the net was created from.  The net must outlive it.
    layout: [{'name', 'shape', 'offset', 'size', 'conv'}] one per parameter in net.common.plain_module_order, `shape` torch's
    ((Cout, Cin, 3, 3) or (C,)); a conv weight lies as [3][3][Cin][Cout] at its offset."""
    KIND = "cls"

    @staticmethod
    def _shape_layout(ent):
        layout = []
        for e in ent:
            conv = e.kh == 3
            layout.append({"name": e.name.decode(), "conv": conv, "shape": (e.Cout, e.Cin, 3, 3) if conv else (e.Cout,),
                           "offset": e.w_off if conv else e.b_off, "size": 9 * e.Cin * e.Cout if conv else e.Cout})
        return layout

    def backward(self, B, H, W, tape_dev, tape_elems, dfeat_dev, grad_dev, grad_elems=None, ctx=None):
        """wsc_net_backward_cls on the net's own context (the workspace belongs to its stream; `ctx`: another one is an error):
        dfeat_dev float32 [B][h][w][F] -> every element of grad_dev (self.grad_elems floats in self.layout)."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_backward_cls(run.h, self.h, int(B), int(H), int(W), _ptr(tape_dev), int(tape_elems), _ptr(dfeat_dev),
                                                 _ptr(grad_dev), self._elems(grad_elems)))

    def backward_drop(self, B, H, W, tape_dev, tape_elems, dfeat_dev, dfeat_elems, grad_dev, drop_prob, seed, step, grad_elems=None, ctx=None):
        """wsc_net_backward_cls_drop: backward() on a tape of Net.forward_cls_train_drop -- WITH THAT PASS'S (drop_prob, seed, step);
        dfeat_dev holds dfeat_elems floats, the shape of that pass's feat."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_backward_cls_drop(run.h, self.h, int(B), int(H), int(W), _ptr(tape_dev), int(tape_elems), _ptr(dfeat_dev),
                                                      _ptr(grad_dev), self._elems(grad_elems), int(dfeat_elems), float(drop_prob),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)))

    # ---- the update half: the training layout (wsc_cls_param_layout), the Nesterov step, the repack -------------------------------
    def _param_query(self):
        if getattr(self, "_param_layout", None) is None:
            ent, (elems,) = _two_call(self.ctx._lib.wsc_cls_param_layout, (self.h,), GradEntry, 1)
            layout = self._shape_layout(ent)
            for d, e in zip(layout, ent):
                d["linear"] = e.kh == 1
                if d["linear"]:  # the classifier's Linear: torch's [C][F], the one matrix that is not transposed
                    d.update(shape=(e.Cout, e.Cin), offset=e.w_off, size=e.Cin * e.Cout)
            self._param_layout, self._param_elems = layout, elems
        return self._param_layout, self._param_elems

    @property
    def param_layout(self):
        """`layout`, then '<root>.classifier.0.weight' ((C, F), lying as it is: 'linear' True) and, if the net has one,
        '<root>.classifier.0.bias': the layout of the parameter, gradient and momentum buffers of a training step"""
        return self._param_query()[0]

    @property
    def param_elems(self):
        return self._param_query()[1]

    @staticmethod
    def fields(layout):
        """torch's OIHW 3 x 3 weights stored as [3][3][Cin][Cout]; the vectors and the classifier's Linear [C][F] as they lie, the
        classifier's two tensors cut to their first C rows"""
        return _named_fields(layout, (2, 3, 1, 0))

    def flat_params(self, state_dict):
        """The trainable tensors of a state dict ({name: array in torch's shape}; other keys are ignored) -> one float32 array of
        param_elems floats in `param_layout`: the host form of what sgd_step and load_params take."""
        return flatten(state_dict, self.fields(self.param_layout), self.param_elems)

    def sgd_step(self, param_dev, grad_dev, mom_dev, lr, momentum=0.9, nesterov=True, elems=None, ctx=None):
        """wsc_cls_sgd_step on three buffers of param_elems floats in `param_layout`: v = momentum m - lr g; m = v;
        p = (p + momentum v) - lr g (nesterov) or p + v, every product, sum and difference one fp32 rounding."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_cls_sgd_step(run.h, self.h, _ptr(param_dev), _ptr(grad_dev), _ptr(mom_dev),
                                             int(self.param_elems if elems is None else elems), float(lr), float(momentum),
                                             int(nesterov)))

    def load_params(self, param_dev, run_dev=None, elems=None, net=None, ctx=None):
        """wsc_net_cls_load_params: the packed conv rows, BatchNorm's gamma / beta, the inference folds (from run_dev, the running
        statistics of forward_cls_train; None leaves them), the classifier, VGG16's CAM head and this object's data-gradient
        kernels rewritten on the device from the flat parameter buffer.  The net must not be in use on another stream."""
        run = ctx or self.ctx
        check(self.ctx._lib.wsc_net_cls_load_params(run.h, (net or self.net).h, self.h, _ptr(param_dev),
                                                    int(self.param_elems if elems is None else elems), _ptr(run_dev)))


def batch_norm_train_nhwc(ctx, a_dev, M, C, gamma_dev, beta_dev, eps, keep, unbiased, run_dev, stats_dev, y_dev):
    """wsc_batch_norm_train_nhwc: a_dev [M][C] -> stats_dev [C][2] {mean, rstd}, y_dev [M][C]; run_dev None or [2][C], updated in
    place with `keep` the weight of the old value; gamma_dev / beta_dev on the device."""
    check(ctx._lib.wsc_batch_norm_train_nhwc(ctx.h, _ptr(a_dev), int(M), int(C), _ptr(gamma_dev), _ptr(beta_dev), float(eps), float(keep),
                                             int(bool(unbiased)), _ptr(run_dev), _ptr(stats_dev), _ptr(y_dev)))


def batch_norm_grad_nhwc(ctx, a_dev, stats_dev, gamma_dev, dy_dev, M, C, da_dev, dgamma_dev, dbeta_dev):
    """wsc_batch_norm_grad_nhwc: da_dev [M][C], dgamma_dev [C], dbeta_dev [C] from the input, the taped statistics and dy_dev."""
    check(ctx._lib.wsc_batch_norm_grad_nhwc(ctx.h, _ptr(a_dev), _ptr(stats_dev), _ptr(gamma_dev), _ptr(dy_dev), int(M), int(C), _ptr(da_dev),
                                            _ptr(dgamma_dev), _ptr(dbeta_dev)))


def batch_norm_train_drop_nhwc(ctx, a_dev, M, C, gamma_dev, beta_dev, eps, keep, unbiased, run_dev, stats_dev, y_dev, drop_prob, seed, step,
                               site):
    """wsc_batch_norm_train_drop_nhwc: batch_norm_train_nhwc with y_dev the dropped, scaled output (keep-mask of (seed, step, site))."""
    check(ctx._lib.wsc_batch_norm_train_drop_nhwc(ctx.h, _ptr(a_dev), int(M), int(C), _ptr(gamma_dev), _ptr(beta_dev), float(eps), float(keep),
                                                  int(bool(unbiased)), _ptr(run_dev), _ptr(stats_dev), _ptr(y_dev), float(drop_prob),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(site)))


def batch_norm_grad_drop_nhwc(ctx, a_dev, stats_dev, gamma_dev, dy_dev, M, C, da_dev, dgamma_dev, dbeta_dev, drop_prob, seed, step, site):
    """wsc_batch_norm_grad_drop_nhwc: batch_norm_grad_nhwc with dy_dev the gradient BEHIND the dropout (the mask is regenerated)."""
    check(ctx._lib.wsc_batch_norm_grad_drop_nhwc(ctx.h, _ptr(a_dev), _ptr(stats_dev), _ptr(gamma_dev), _ptr(dy_dev), int(M), int(C),
                                                 _ptr(da_dev), _ptr(dgamma_dev), _ptr(dbeta_dev), float(drop_prob),
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(site)))


def pool_tf_grad_nhwc(ctx, x_dev, dy_dev, N, H, W, C, k, stride, same, dx_dev):
    """wsc_pool_tf_grad_nhwc: the gradient of pool_tf_nhwc with respect to its input."""
    check(ctx._lib.wsc_pool_tf_grad_nhwc(ctx.h, _ptr(x_dev), _ptr(dy_dev), int(N), int(H), int(W), int(C), int(k), int(stride), int(bool(same)),
                                         _ptr(dx_dev)))


def maxpool_grad_nhwc(ctx, x_dev, dy_dev, N, H, W, C, k, stride, pad, dx_dev):
    """wsc_maxpool_grad_nhwc: the gradient of maxpool_nhwc (torch's MaxPool2d(k, stride, pad)) with respect to its input."""
    check(ctx._lib.wsc_maxpool_grad_nhwc(ctx.h, _ptr(x_dev), _ptr(dy_dev), int(N), int(H), int(W), int(C), int(k), int(stride), int(pad),
                                         _ptr(dx_dev)))


def channel_mean_nchw(ctx, x_dev, N, C, H, W, out_dev, sub=None):
    """wsc_channel_mean_nchw: out_dev[c] (float64) = mean over (n, h, w) of x_dev float32 [N][C][H][W], in double in one fixed
    order, minus sub[c] (host floats, or None)."""
    s = None if sub is None else np.ascontiguousarray(sub, dtype=np.float32)
    if s is not None and s.shape != (int(C),):
        raise ValueError("channel_mean_nchw: sub has shape %r, expected (%d,)" % (s.shape, C))
    check(ctx._lib.wsc_channel_mean_nchw(ctx.h, _ptr(x_dev), int(N), int(C), int(H), int(W), _ptr(s), _ptr(out_dev)))


def relu_upsample_grad_nhwc(ctx, dcat_dev, cat_dev, N, H, W, C, up, Hd, Wd, Ctot, coff, dy_dev):
    """wsc_relu_upsample_grad_nhwc: dy_dev [N][H][W][C] from dcat_dev and the concat values cat_dev, both [N][Hd][Wd][Ctot]."""
    check(ctx._lib.wsc_relu_upsample_grad_nhwc(ctx.h, _ptr(dcat_dev), _ptr(cat_dev), int(N), int(H), int(W), int(C), int(up), int(Hd), int(Wd),
                                               int(Ctot), int(coff), _ptr(dy_dev)))


def group_norm_grad_nhwc(ctx, z_dev, dy_dev, N, H, W, C, gamma, G, eps, dz_dev, dgamma_dev, dbeta_dev):
    """wsc_group_norm_grad_nhwc: dz_dev [N][H][W][C], dgamma_dev [C], dbeta_dev [C] of GroupNorm(G, C); gamma on the host."""
    gamma = np.ascontiguousarray(gamma, dtype=np.float32)
    assert gamma.shape == (C,)
    check(ctx._lib.wsc_group_norm_grad_nhwc(ctx.h, _ptr(z_dev), _ptr(dy_dev), int(N), int(H), int(W), int(C), _ptr(gamma), int(G), float(eps),
                                            _ptr(dz_dev), _ptr(dgamma_dev), _ptr(dbeta_dev)))


def conv2d_wgrad_nhwc(ctx, x_dev, dy_dev, N, H, W, Cin, Cout, k, dil, splits, dw_dev, db_dev):
    """wsc_conv2d_wgrad_nhwc: dw_dev [k][k][Cin][Cout], db_dev [Cout] of a stride-1 SAME convolution; splits 0 = the launcher's."""
    check(ctx._lib.wsc_conv2d_wgrad_nhwc(ctx.h, _ptr(x_dev), _ptr(dy_dev), int(N), int(H), int(W), int(Cin), int(Cout), int(k), int(dil),
                                         int(splits), _ptr(dw_dev), _ptr(db_dev)))


def conv2d_dgrad_nhwc(ctx, dy_dev, w, N, H, W, Cin, Cout, k, dil, dx_dev):
    """wsc_conv2d_dgrad_nhwc: dx_dev [N][H][W][Cin] from dy_dev [N][H][W][Cout] and the host weights w [k][k][Cin][Cout]."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.shape == (k, k, Cin, Cout)
    check(ctx._lib.wsc_conv2d_dgrad_nhwc(ctx.h, _ptr(dy_dev), _ptr(w), int(N), int(H), int(W), int(Cin), int(Cout), int(k), int(dil),
                                         _ptr(dx_dev)))


def relu_bias_grad(ctx, y_dev, dy_dev, M, C, dz_dev, db_dev):
    """wsc_relu_bias_grad: dz = dy [y > 0] (y_dev None: dz = dy), db = the column sums of dz."""
    check(ctx._lib.wsc_relu_bias_grad(ctx.h, _ptr(y_dev), _ptr(dy_dev), int(M), int(C), _ptr(dz_dev), _ptr(db_dev)))


def relu_bias_grad_scaled(ctx, y_dev, dy_dev, M, C, scale, dz_dev, db_dev):
    """wsc_relu_bias_grad_scaled: dz = dy scale [y > 0] (one fp32 rounding), db = the column sums of dz."""
    check(ctx._lib.wsc_relu_bias_grad_scaled(ctx.h, _ptr(y_dev), _ptr(dy_dev), int(M), int(C), float(scale), _ptr(dz_dev), _ptr(db_dev)))


def seg_dropout_f32(ctx, x_dev, elems, first, drop_prob, seed, step, site, y_dev, keep_dev=None):
    """wsc_seg_dropout_f32: the dropout kernel on plain float32; x_dev[0] is element `first` of the logical tensor, keep_dev
    (optional) receives one byte per element."""
    check(ctx._lib.wsc_seg_dropout_f32(ctx.h, _ptr(x_dev), int(elems), int(first), float(drop_prob), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step),
                                       int(site), _ptr(y_dev), _ptr(keep_dev)))


def pool_same_grad_nhwc(ctx, x_dev, dy_dev, N, H, W, C, avg, stride, dx_dev):
    """wsc_pool_same_grad_nhwc: the gradient of pool_same_nhwc with respect to its input."""
    check(ctx._lib.wsc_pool_same_grad_nhwc(ctx.h, _ptr(x_dev), _ptr(dy_dev), int(N), int(H), int(W), int(C), int(bool(avg)), int(stride),
                                           _ptr(dx_dev)))


def _key_table(keys_per_image, B=None):
    """The int sequences of the first B images (default: all) -> (keys, key_off): the int32 keys one image after the other
    (length >= 1, so that the array always has an address) and the int32 offsets [0, n_0, n_0 + n_1, ...] of the images."""
    per = [np.asarray(k, dtype=np.int32).reshape(-1) for k in list(keys_per_image)[:B]]
    key_off = np.zeros(len(per) + 1, dtype=np.int32)
    key_off[1:] = np.cumsum([len(k) for k in per])
    return np.concatenate(per + [np.zeros(0 if key_off[-1] else 1, np.int32)]), key_off


def _size_table(sizes, B):
    """B (height, width) pairs -> C-contiguous int32 (B, 2)."""
    return np.ascontiguousarray(sizes, dtype=np.int32).reshape(B, 2)


def cam_postprocess(ctx, cam_dev, B, C, h, w, sizes, keys_per_image, strided_dev=None, highres_dev=None):
    """Batched make_cam tail.  sizes: [(H0, W0)], keys_per_image: list of int sequences.

    Returns (strided_dev, highres_dev, strided_off, highres_off, shapes) where shapes[b] =
    (K, h4, w4, H0, W0); buffers are allocated when not given.
    """
    size_hw = _size_table(sizes, B)
    keys, key_off = _key_table(keys_per_image, B)
    s_off = np.zeros(B, dtype=np.int64)
    h_off = np.zeros(B, dtype=np.int64)
    shapes = []
    s_tot = 0
    h_tot = 0
    for b in range(B):
        H0, W0 = int(size_hw[b, 0]), int(size_hw[b, 1])
        h4, w4 = (H0 - 1) // 4 + 1, (W0 - 1) // 4 + 1
        K = int(key_off[b + 1] - key_off[b])
        s_off[b] = s_tot
        h_off[b] = h_tot
        s_tot += K * h4 * w4
        h_tot += K * H0 * W0
        shapes.append((K, h4, w4, H0, W0))
    if strided_dev is None:
        strided_dev = ctx.alloc(max(s_tot, 1) * 4)
    if highres_dev is None:
        highres_dev = ctx.alloc(max(h_tot, 1) * 4)
    check(ctx._lib.wsc_cam_postprocess(ctx.h, _ptr(cam_dev), B, C, h, w, size_hw.ctypes.data, keys.ctypes.data,
                                       key_off.ctypes.data, s_off.ctypes.data, h_off.ctypes.data,
                                       _ptr(strided_dev), _ptr(highres_dev)))
    return strided_dev, highres_dev, s_off, h_off, shapes


def conv2d_nchw(ctx, x_dev, N, Cin, H, W, w, stride, pad, scale=None, shift=None, residual_dev=None, relu=False,
                precision=PREC_BF16, y_dev=None, dil=1):
    """One conv layer through the production kernel (test/diagnostic entry).  dil: the dilation (wsc_conv2d_nchw_dil; 1 through
    that entry is wsc_conv2d_nchw itself)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    Cout, _, kh, kw = w.shape
    dil = int(dil)
    Ho, Wo = (H + 2 * pad - ((kh - 1) * dil + 1)) // stride + 1, (W + 2 * pad - ((kw - 1) * dil + 1)) // stride + 1
    if y_dev is None:
        y_dev = ctx.alloc(N * Cout * Ho * Wo * 4)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32)
    if dil == 1:
        check(ctx._lib.wsc_conv2d_nchw(ctx.h, _ptr(x_dev), N, Cin, H, W, w.ctypes.data, Cout, kh, kw, stride, pad,
                                       None if sc is None else sc.ctypes.data, None if sh is None else sh.ctypes.data,
                                       _ptr(residual_dev), int(relu), precision, _ptr(y_dev)))
    else:
        conv2d_nchw_dil(ctx, x_dev, N, Cin, H, W, w, stride, pad, dil, sc, sh, residual_dev, relu, precision, y_dev)
    return y_dev, (N, Cout, Ho, Wo)


def conv2d_nchw_dil(ctx, x_dev, N, Cin, H, W, w, stride, pad, dil, scale, shift, residual_dev, relu, precision, y_dev):
    """wsc_conv2d_nchw_dil as it is (conv2d_nchw(dil=) routes here for dil > 1; a test calls it with dil = 1)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    Cout, _, kh, kw = w.shape
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32)
    check(ctx._lib.wsc_conv2d_nchw_dil(ctx.h, _ptr(x_dev), N, Cin, H, W, w.ctypes.data, Cout, kh, kw, stride, pad, int(dil),
                                       None if sc is None else sc.ctypes.data, None if sh is None else sh.ctypes.data,
                                       _ptr(residual_dev), int(relu), precision, _ptr(y_dev)))


def resize_bilinear_tf(ctx, src_dev, B, h, w, C, H, W, dst_dev=None):
    """TensorFlow 1.x tf.image.resize_bilinear(align_corners=False) on NHWC float32 (wsc_resize_bilinear_tf):
    src_dev [B][h][w][C] -> dst_dev [B][H][W][C] (allocated when not given)."""
    if dst_dev is None:
        dst_dev = ctx.alloc(B * H * W * C * 4)
    check(ctx._lib.wsc_resize_bilinear_tf(ctx.h, _ptr(src_dev), int(B), int(h), int(w), int(C), _ptr(dst_dev), int(H), int(W)))
    return dst_dev


def pool_same_nhwc(ctx, x_dev, N, H, W, C, avg, stride, precision, y_dev=None):
    """One TF-SAME 3x3 pool of the SEC / DSRG nets on float32 NHWC (wsc_pool_same_nhwc) -> (y_dev, (N, Ho, Wo, C))."""
    Ho, Wo = -(-H // stride), -(-W // stride)
    if y_dev is None:
        y_dev = ctx.alloc(N * Ho * Wo * C * 4)
    check(ctx._lib.wsc_pool_same_nhwc(ctx.h, _ptr(x_dev), int(N), int(H), int(W), int(C), int(bool(avg)), int(stride), int(precision),
                                      _ptr(y_dev)))
    return y_dev, (N, Ho, Wo, C)


def pool_tf_nhwc(ctx, x_dev, N, H, W, C, k, stride, same, precision, y_dev=None):
    """One TF / Keras MaxPooling2D(k, stride, 'same' if same else 'valid') on float32 NHWC (wsc_pool_tf_nhwc) ->
    (y_dev, (N, Ho, Wo, C)); the output size is net.common.pooled_size's (a VALID window wider than the map: WscError)."""
    from .net.common import pooled_size

    row = (int(k), int(stride), "same" if same else "valid")
    try:
        Ho, Wo = pooled_size(H, [row]), pooled_size(W, [row])
    except ValueError:
        Ho = Wo = 0  # (no such output: the library says so before it launches anything)
    if y_dev is None:
        y_dev = ctx.alloc(max(N * Ho * Wo * C, 1) * 4)
    check(ctx._lib.wsc_pool_tf_nhwc(ctx.h, _ptr(x_dev), int(N), int(H), int(W), int(C), int(k), int(stride), int(same),
                                    int(precision), _ptr(y_dev)))
    return y_dev, (N, Ho, Wo, C)


def group_norm_nhwc(ctx, x_dev, N, H, W, C, gamma, beta, G, eps, up, relu, Hd, Wd, Ctot, coff, precision, y_dev):
    """One IRNet head after its convolution (wsc_group_norm_nhwc): GroupNorm(G, C) of float32 NHWC x_dev, bilinear x `up`, crop to
    Hd x Wd, ReLU if `relu`, into channels [coff, coff + C) of y_dev float32 [N][Hd][Wd][Ctot] -- which is read first: its other
    channels come back rounded to the precision.  gamma / beta: host arrays [C]."""
    g = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float32)
    b = None if beta is None else np.ascontiguousarray(beta, dtype=np.float32)
    check(ctx._lib.wsc_group_norm_nhwc(ctx.h, _ptr(x_dev), int(N), int(H), int(W), int(C), _ptr(g), _ptr(b), int(G), float(eps), int(up),
                                       int(bool(relu)), int(Hd), int(Wd), int(Ctot), int(coff), int(precision), _ptr(y_dev)))
    return y_dev, (N, Hd, Wd, Ctot)


def maxpool_nhwc(ctx, x_dev, N, H, W, C, k, stride, pad, precision, y_dev=None):
    """nn.MaxPool2d(k, stride, pad) of the torch-side nets on float32 NHWC (wsc_maxpool_nhwc) -> (y_dev, (N, Ho, Wo, C))."""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if y_dev is None:
        y_dev = ctx.alloc(max(N * Ho * Wo * C, 1) * 4)
    check(ctx._lib.wsc_maxpool_nhwc(ctx.h, _ptr(x_dev), int(N), int(H), int(W), int(C), int(k), int(stride), int(pad), int(precision),
                                    _ptr(y_dev)))
    return y_dev, (N, Ho, Wo, C)


def gap_linear_sigmoid(ctx, feat_dev, B, hw, F, w, bias, sample_stride, precision, score_dev=None):
    """The classifier branch (wsc_gap_linear_sigmoid): feat_dev float32 [B * sample_stride][|hw|][F] -> (score_dev, (B, C)), the
    sigmoid of Linear(w [C][F], bias [C] or None) on the mean (hw > 0) or the maximum (hw < 0) over the positions."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    C = w.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    if score_dev is None:
        score_dev = ctx.alloc(max(B * C, 1) * 4)
    check(ctx._lib.wsc_gap_linear_sigmoid(ctx.h, _ptr(feat_dev), int(B), int(hw), int(F), _ptr(w), _ptr(b), int(C), int(sample_stride),
                                          int(precision), _ptr(score_dev)))
    return score_dev, (B, C)


def cam_flip_add(ctx, head_dev, B, h, w, C, Cs, cam_dev=None):
    """cam [B][C][h][w] = relu(head[2b]) + relu(head[2b + 1]).flip(-1) of float32 NHWC head_dev [2B][h][w][Cs] (wsc_cam_flip_add)."""
    if cam_dev is None:
        cam_dev = ctx.alloc(max(B * C * h * w, 1) * 4)
    check(ctx._lib.wsc_cam_flip_add(ctx.h, _ptr(head_dev), int(B), int(h), int(w), int(C), int(Cs), _ptr(cam_dev)))
    return cam_dev, (B, C, h, w)


def irn_edge_finish(ctx, e_dev, He, We, d_dev, Hd, Wd, B, fh, fw, ms0, ms1, edge_dev=None, dp_dev=None):
    """The end of EdgeDisplacement.forward (wsc_irn_edge_finish): e_dev [2B][He][We], d_dev [2B][Hd][Wd][2] ->
    (edge_dev [B][fh][fw], dp_dev [B][2][fh][fw])."""
    n = max(B * fh * fw, 1)
    if edge_dev is None:
        edge_dev = ctx.alloc(n * 4)
    if dp_dev is None:
        dp_dev = ctx.alloc(2 * n * 4)
    check(ctx._lib.wsc_irn_edge_finish(ctx.h, _ptr(e_dev), int(He), int(We), _ptr(d_dev), int(Hd), int(Wd), int(B), int(fh), int(fw),
                                       float(ms0), float(ms1), _ptr(edge_dev), _ptr(dp_dev)))
    return edge_dev, dp_dev


def fc8_softmax(ctx, fc8_devs, M, C, prob_dev, min_prob=1e-4, sum_dev=None):
    """fc8-softmax of the sum of 1 .. 4 float32 [M][C] logit arrays on the device (wsc_fc8_softmax)."""
    ptrs = (_vp * len(fc8_devs))(*[_ptr(d) for d in fc8_devs])
    check(ctx._lib.wsc_fc8_softmax(ctx.h, ptrs, len(fc8_devs), int(M), int(C), float(min_prob), _ptr(sum_dev), _ptr(prob_dev)))


def cam_eval_confusion(ctx, highres_dev, sizes, keys_per_image, highres_off, bg_thres, gt_dev, n_class, confusion_dev,
                       pred_dev=None, ignore_label=255):
    """Accumulates the eval_cam confusion matrix of a batch into confusion_dev (int64 [n_class][n_class])."""
    B = len(sizes)
    size_hw = _size_table(sizes, B)
    keys, key_off = _key_table(keys_per_image, B)
    h_off = np.ascontiguousarray(highres_off, dtype=np.int64)
    check(ctx._lib.wsc_cam_eval_confusion(ctx.h, _ptr(highres_dev), B, size_hw.ctypes.data, keys.ctypes.data,
                                          key_off.ctypes.data, h_off.ctypes.data, float(bg_thres), _ptr(gt_dev),
                                          int(n_class), int(ignore_label), _ptr(pred_dev), _ptr(confusion_dev)))


def cam_eval_confusion_nn(ctx, maps_dev, src_sizes, out_sizes, keys_per_image, maps_off, gt_dev, n_class, confusion_dev,
                          pred_dev=None, ignore_label=255):
    """ADP / DeepGlobe eval_cam branch: keys[argmax(maps)] at the maps' size, cv2 nearest resize to out_sizes, confusion."""
    B = len(src_sizes)
    src_hw = _size_table(src_sizes, B)
    out_hw = _size_table(out_sizes, B)
    keys, key_off = _key_table(keys_per_image, B)
    m_off = np.ascontiguousarray(maps_off, dtype=np.int64)
    check(ctx._lib.wsc_cam_eval_confusion_nn(ctx.h, _ptr(maps_dev), B, src_hw.ctypes.data, out_hw.ctypes.data, keys.ctypes.data,
                                             key_off.ctypes.data, m_off.ctypes.data, _ptr(gt_dev), int(n_class),
                                             int(ignore_label), _ptr(pred_dev), _ptr(confusion_dev)))


def label_confusion_nn(ctx, labels_dev, src_sizes, out_sizes, labels_off, gt_dev, n_class, confusion_dev, pred_dev=None,
                       ignore_label=255):
    """HSN evaluation tail: int32 label maps -> cv2 nearest resize to out_sizes -> confusion[gt][pred] (accumulated)."""
    B = len(src_sizes)
    src_hw = _size_table(src_sizes, B)
    out_hw = _size_table(out_sizes, B)
    off = np.ascontiguousarray(labels_off, dtype=np.int64)
    check(ctx._lib.wsc_label_confusion_nn(ctx.h, _ptr(labels_dev), B, src_hw.ctypes.data, out_hw.ctypes.data, off.ctypes.data,
                                          _ptr(gt_dev), int(n_class), int(ignore_label), _ptr(pred_dev), _ptr(confusion_dev)))


def render_labels(ctx, labels_dev, label_dtype, src_sizes, out_sizes, labels_off, out_off, palette, other_rgb, colour_dev,
                  mid_sizes=None, img_dev=None, blend=None, overlay_dev=None):
    """The debug images of a ragged batch (wsc_render_labels): label maps (uint8 or int32, per `label_dtype`) -> cv2 nearest
    resize in one or two stages -> palette lookup into colour_dev and, with overlay_dev, the blend-table overlay on img_dev.
    labels_off in elements, out_off in bytes; `blend`: uint8 (n_colours + 1, 3, 256) of wsscam.render.blend_table."""
    B = len(src_sizes)
    src_hw, out_hw = _size_table(src_sizes, B), _size_table(out_sizes, B)
    mid_hw = _size_table(mid_sizes, B) if mid_sizes is not None else None
    l_off, o_off = np.ascontiguousarray(labels_off, dtype=np.int64), np.ascontiguousarray(out_off, dtype=np.int64)
    assert l_off.shape == (B,) and o_off.shape == (B,)
    pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 3)
    other = np.ascontiguousarray(other_rgb, dtype=np.uint8).reshape(3)
    kind = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1}[np.dtype(label_dtype)]
    if blend is not None:
        blend = np.ascontiguousarray(blend, dtype=np.uint8)
        assert blend.shape == (len(pal) + 1, 3, 256), blend.shape
    check(ctx._lib.wsc_render_labels(ctx.h, _ptr(labels_dev), kind, B, src_hw.ctypes.data,
                                     None if mid_hw is None else mid_hw.ctypes.data, out_hw.ctypes.data, l_off.ctypes.data,
                                     o_off.ctypes.data, pal.ctypes.data, len(pal), other.ctypes.data, _ptr(img_dev), _ptr(blend),
                                     _ptr(colour_dev), _ptr(overlay_dev)))


def sem_seg_finish(ctx, rw_dev, rw_off, khw, up_hw, out_hw, keys_per_image, has_bg, bg_thres, label_dev):
    """make_sem_seg_labels tail on the device: upsample + crop + / max + [bg pad] + argmax + keys -> packed uint8 labels."""
    B = len(khw)
    keys, key_off = _key_table(keys_per_image, B)
    off = np.ascontiguousarray(rw_off, dtype=np.int64)
    a, u, o = (np.ascontiguousarray(v, dtype=np.int32).reshape(B, -1) for v in (khw, up_hw, out_hw))
    check(ctx._lib.wsc_sem_seg_finish(ctx.h, _ptr(rw_dev), B, off.ctypes.data, a.ctypes.data, u.ctypes.data, o.ctypes.data,
                                      keys.ctypes.data, key_off.ctypes.data, int(bool(has_bg)), float(bg_thres), _ptr(label_dev)))


def unary_from_maps(ctx, maps_dev, B, C, N, bg_value, unary_dev):
    check(ctx._lib.wsc_unary_from_maps(ctx.h, _ptr(maps_dev), B, C, N, float(bg_value), _ptr(unary_dev)))


def cam_unary(ctx, cam_dev, B, C, h, w, H0, W0, bg_value, unary_dev, pixel_major=False):
    """cam_postprocess (all classes at H0 x W0) + unary_from_maps without the intermediate maps in HBM.
    pixel_major: unaries as [B][H0*W0][Mp] (Mp = 4 ceil((C+1)/4)) for Crf.inference(..., pixel_major=True)."""
    fn = ctx._lib.wsc_cam_unary_pm if pixel_major else ctx._lib.wsc_cam_unary
    check(fn(ctx.h, _ptr(cam_dev), B, C, h, w, H0, W0, float(bg_value), _ptr(unary_dev)))


def cam_sum_scales(ctx, cam_dev, n_images, n_scales, map_elems, out_dev):
    """out[b] = sum_s cam[b * n_scales + s] (make_cam.py:62-69 for equal-size scales; see include/wsscam.h)."""
    check(ctx._lib.wsc_cam_sum_scales(ctx.h, _ptr(cam_dev), int(n_images), int(n_scales), int(map_elems), _ptr(out_dev)))


def bilinear_resize(ctx, src_dev, C, h, w, dst_dev, H, W):
    check(ctx._lib.wsc_bilinear_resize(ctx.h, _ptr(src_dev), C, h, w, _ptr(dst_dev), H, W))


class Crf:
    """wsc_crf: lattices of a batch of images (DenseCRF2D + addPairwise*)."""

    def __init__(self, ctx, rgb_dev, B, H, W, g_sxy, bi_sxy, bi_srgb):
        self.ctx = ctx
        self.B, self.H, self.W = B, H, W
        h = _vp()
        check(ctx._lib.wsc_crf_create(ctx.h, _ptr(rgb_dev), B, H, W, float(g_sxy), float(bi_sxy), float(bi_srgb),
                                      ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx._lib.wsc_crf_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lattice_sizes(self):
        vg = np.zeros(self.B, dtype=np.int32)
        vb = np.zeros(self.B, dtype=np.int32)
        check(self.ctx._lib.wsc_crf_lattice_sizes(self.ctx.h, self.h, vg.ctypes.data, vb.ctypes.data))
        return vg, vb

    def gaussian_on_chip(self, M):
        """True when the update kernel blurs the Gaussian lattice itself for an M-class inference (wsc_crf_gaussian_on_chip)."""
        return bool(self.ctx._lib.wsc_crf_gaussian_on_chip(self.h, int(M)))

    def inference(self, unary_dev, M, g_compat, bi_compat, n_iters, q_dev=None, argmax_dev=None, ctx=None, pixel_major=False):
        """ctx: the context (stream, workspace) to run the mean-field loop on; defaults to the one the
        lattices were built on.  When it differs, the caller orders the two with ctx.wait_for(build_ctx).
        pixel_major: unary_dev is [B][H*W][Mp] (cam_unary(..., pixel_major=True)), read in place."""
        run = ctx or self.ctx
        fn = self.ctx._lib.wsc_crf_inference_pm if pixel_major else self.ctx._lib.wsc_crf_inference
        check(fn(run.h, self.h, _ptr(unary_dev), M, float(g_compat), float(bi_compat), int(n_iters), _ptr(q_dev),
                 _ptr(argmax_dev)))


def _ptr_array(ptrs):
    """list of DeviceBuffer / int addresses / None -> ctypes array of void* (kept alive by the caller)."""
    arr = (ctypes.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = None if p is None else (p.ptr if hasattr(p, "ptr") else int(p))
    return arr


class CrfV:
    """wsc_crf_v: lattices of a RAGGED batch -- every image its own (H, W) and, at inference, its own class count.
    rgb_ptrs: one device pointer (DeviceBuffer or address) per image, uint8 [H_b][W_b][3]; sizes: [(H_b, W_b)]."""

    def __init__(self, ctx, rgb_ptrs, sizes, g_sxy, bi_sxy, bi_srgb):
        self.ctx = ctx
        self.B = len(rgb_ptrs)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        assert len(self.sizes) == self.B
        hw = _size_table(self.sizes, self.B)
        arr = _ptr_array(rgb_ptrs)
        h = _vp()
        check(ctx._lib.wsc_crf_v_create(ctx.h, arr, hw.ctypes.data, self.B, float(g_sxy), float(bi_sxy), float(bi_srgb),
                                        ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx._lib.wsc_crf_v_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_groups(self):
        return int(self.ctx._lib.wsc_crf_v_num_groups(self.h))

    def inference(self, unary_ptrs, Ms, g_compat, bi_compat, n_iters, q_ptrs=None, argmax_ptrs=None, ctx=None):
        """unary_ptrs[b]: float32 [M_b][H_b*W_b] on the device; q_ptrs / argmax_ptrs: per-image outputs (lists, or None)."""
        run = ctx or self.ctx
        m = np.ascontiguousarray(Ms, dtype=np.int32)
        assert len(unary_ptrs) == self.B and len(m) == self.B
        ua = _ptr_array(unary_ptrs)
        qa = _ptr_array(q_ptrs) if q_ptrs is not None else None
        aa = _ptr_array(argmax_ptrs) if argmax_ptrs is not None else None
        check(self.ctx._lib.wsc_crf_v_inference(run.h, self.h, ua, m.ctypes.data, float(g_compat), float(bi_compat), int(n_iters),
                                                qa, aa))


def rw_propagate(ctx, x_dev, edge_dev, K, h, w, dirs, path_start, path_yx, beta, n_steps, rw_dev=None):
    """wsc_rw_propagate: x_dev [K][h][w], edge_dev [h][w] device buffers -> rw_dev [K][h][w] (allocated if None)."""
    import numpy as np

    dirs = np.ascontiguousarray(dirs, dtype=np.int32)
    path_start = np.ascontiguousarray(path_start, dtype=np.int32)
    path_yx = np.ascontiguousarray(path_yx, dtype=np.int32)
    if rw_dev is None:
        rw_dev = ctx.alloc(K * h * w * 4)
    check(ctx._lib.wsc_rw_propagate(ctx.h, _ptr(x_dev), _ptr(edge_dev), K, h, w, dirs.ctypes.data_as(_vp),
                                    path_start.ctypes.data_as(_vp), path_yx.ctypes.data_as(_vp), int(dirs.shape[0]),
                                    float(beta), int(n_steps), _ptr(rw_dev)))
    return rw_dev


def rw_propagate_batch(ctx, x_dev, edge_dev, Ks, hs, ws, dirs, path_start, path_yx, beta, n_steps, rw_dev=None):
    """wsc_rw_propagate_batch: packed [K_b][h_b][w_b] blocks / [h_b][w_b] edge maps of several images."""
    import numpy as np

    Ks, hs, ws = (np.ascontiguousarray(v, dtype=np.int32) for v in (Ks, hs, ws))
    dirs = np.ascontiguousarray(dirs, dtype=np.int32)
    path_start = np.ascontiguousarray(path_start, dtype=np.int32)
    path_yx = np.ascontiguousarray(path_yx, dtype=np.int32)
    if rw_dev is None:
        rw_dev = ctx.alloc(int((Ks.astype(np.int64) * hs * ws).sum()) * 4)
    check(ctx._lib.wsc_rw_propagate_batch(ctx.h, int(len(Ks)), Ks.ctypes.data_as(_vp), hs.ctypes.data_as(_vp),
                                          ws.ctypes.data_as(_vp), _ptr(x_dev), _ptr(edge_dev), dirs.ctypes.data_as(_vp),
                                          path_start.ctypes.data_as(_vp), path_yx.ctypes.data_as(_vp),
                                          int(dirs.shape[0]), float(beta), int(n_steps), _ptr(rw_dev)))
    return rw_dev



# ---- HistoSegNet post-processing (csrc/hsn.hip) -------------------------------------------------------------------
def hsn_gradcam_post(ctx, cams_nhwc_dev, B, h, w, C, S, gate_dev, out_dev, out_channels=0, out_first=0):
    check(ctx._lib.wsc_hsn_gradcam_post(ctx.h, _ptr(cams_nhwc_dev), B, h, w, C, S, _ptr(gate_dev), _ptr(out_dev),
                                        int(out_channels), int(out_first)))


def hsn_voc_background(ctx, Hbg_dev, B, Cb, N, y_dev, Ctot):
    check(ctx._lib.wsc_hsn_voc_background(ctx.h, _ptr(Hbg_dev), B, Cb, N, _ptr(y_dev), Ctot))


def hsn_class_mass(ctx, maps_dev, n_maps, N, mass_dev):
    check(ctx._lib.wsc_hsn_class_mass(ctx.h, _ptr(maps_dev), n_maps, N, _ptr(mass_dev)))


def hsn_background(ctx, rgb_dev, B, H, W, bg_dev, out_hw=None):
    Ho, Wo = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    check(ctx._lib.wsc_hsn_background(ctx.h, _ptr(rgb_dev), B, H, W, Ho, Wo, _ptr(bg_dev)))


def cam_adp_modify(ctx, cam_dev, B, n_sc, C, hw, bg_dev, mode, use, adipose, exc, out_dev):
    """wsc_cam_adp_modify: common_cam.py:31-92 on the device; -> number of output channels (len(use) + 1 + mode)."""
    us = np.ascontiguousarray(use, dtype=np.int32)
    ad = np.ascontiguousarray(adipose, dtype=np.int32)
    ex = np.ascontiguousarray(exc if exc is not None else [], dtype=np.int32)
    check(ctx._lib.wsc_cam_adp_modify(ctx.h, _ptr(cam_dev), int(B), int(n_sc), int(C), int(hw), _ptr(bg_dev), int(mode),
                                      us.ctypes.data, len(us), ad.ctypes.data, len(ad), ex.ctypes.data if len(ex) else None,
                                      len(ex), _ptr(out_dev)))
    return len(us) + 1 + int(mode)


def hsn_cs_gradcam(ctx, H_dev, B, C_all, N, bg_dev, src_of_valid, bg_ind, other_ind, exception_inds, adipose_src, cs_dev,
                   y_dev, mass_dev):
    sv = np.ascontiguousarray(src_of_valid, dtype=np.int32)
    ex = np.ascontiguousarray(exception_inds, dtype=np.int32)
    ad = np.ascontiguousarray(adipose_src if adipose_src is not None else [], dtype=np.int32)
    check(ctx._lib.wsc_hsn_cs_gradcam(ctx.h, _ptr(H_dev), B, C_all, N, _ptr(bg_dev), sv.ctypes.data, len(sv), int(bg_ind),
                                      int(other_ind), ex.ctypes.data if len(ex) else None, len(ex),
                                      ad.ctypes.data if len(ad) else None, len(ad), _ptr(cs_dev), _ptr(y_dev), _ptr(mass_dev)))


def hsn_gather_unary(ctx, maps_dev, chan_off, N, unary_dev):
    co = np.ascontiguousarray(chan_off, dtype=np.int64)
    check(ctx._lib.wsc_hsn_gather_unary(ctx.h, _ptr(maps_dev), co.ctypes.data, len(co), N, _ptr(unary_dev)))


def msf_input_u8(ctx, images_dev, sizes, offsets, S, mean, std, x_dev, pre_div255=False, pair=True):
    """wsc_msf_input_u8: decoded uint8 images (packed HWC blocks at byte `offsets`) -> float32 network input."""
    B = len(sizes)
    size_hw = _size_table(sizes, B)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    m = np.ascontiguousarray(mean, dtype=np.float32)
    sd = np.ascontiguousarray(std, dtype=np.float32)
    check(ctx._lib.wsc_msf_input_u8(ctx.h, _ptr(images_dev), B, size_hw.ctypes.data, off.ctypes.data, int(S), m.ctypes.data,
                                    sd.ctypes.data, int(bool(pre_div255)), int(bool(pair)), _ptr(x_dev)))


def resize_u8(ctx, images_dev, sizes, offsets, out_hw, out_dev):
    """wsc_resize_u8: cv2.resize (INTER_LINEAR, 8-bit fixed point) of packed uint8 HWC images -> uint8 [B][OH][OW][3]."""
    B = len(sizes)
    size_hw = _size_table(sizes, B)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    check(ctx._lib.wsc_resize_u8(ctx.h, _ptr(images_dev), B, size_hw.ctypes.data, off.ctypes.data, int(out_hw[0]), int(out_hw[1]),
                                 _ptr(out_dev)))


def _offset_table(name, offsets, B):
    """B byte offsets -> C-contiguous int64 (B,); anything that is no whole number, negative or of another length is an error"""
    off = np.asarray(offsets)
    if off.shape != (B,) or off.dtype.kind not in "iu":
        raise ValueError("%s: %r %s, expected %d integer byte offsets" % (name, off.shape, off.dtype, B))
    if B and int(off.min()) < 0:
        raise ValueError("%s: negative byte offset" % name)
    return np.ascontiguousarray(off, dtype=np.int64)


def _hw_table(name, sizes, B):
    """B (height, width) pairs of whole numbers >= 1 -> C-contiguous int32 (B, 2)"""
    t = np.asarray(sizes)
    if t.dtype.kind not in "iu" or t.size != 2 * B:
        raise ValueError("%s: %r %s, expected %d (height, width) pairs of integers" % (name, t.shape, t.dtype, B))
    t = t.reshape(B, 2)
    if B and (int(t.min()) < 1 or int(t.max()) > 32768):
        raise ValueError("%s: a side outside 1 .. 32768" % name)
    return np.ascontiguousarray(t, dtype=np.int32)


def pil_resize_u8(ctx, images_dev, sizes, offsets, out_sizes, out_offsets, channels, order, out_dev):
    """wsc_pil_resize_u8: PIL's Image.resize (order 3 bicubic, 0 nearest) of packed uint8 images ([H][W][channels] blocks at byte
    `offsets`) -> uint8 blocks [OH][OW][channels] at byte `out_offsets` of out_dev.  Shapes and dtypes are checked here, before
    any C call."""
    B = len(sizes)
    if not 1 <= B <= 65535:
        raise ValueError("pil_resize_u8: %d images (1 .. 65535)" % B)
    if channels not in (1, 3):
        raise ValueError("pil_resize_u8: channels = %r (1 or 3)" % (channels,))
    size_hw, out_hw = _hw_table("pil_resize_u8: sizes", sizes, B), _hw_table("pil_resize_u8: out_sizes", out_sizes, B)
    off, out_off = _offset_table("pil_resize_u8: offsets", offsets, B), _offset_table("pil_resize_u8: out_offsets", out_offsets, B)
    check(ctx._lib.wsc_pil_resize_u8(ctx.h, _ptr(images_dev), B, size_hw.ctypes.data, off.ctypes.data, out_hw.ctypes.data,
                                     out_off.ctypes.data, int(channels), int(order), _ptr(out_dev)))


IRN_BATCH_PARAMS = ("scaled_h", "scaled_w", "flip", "cont_top", "cont_left", "img_top", "img_left", "ch", "cw")
IRN_STAGE_NONE, IRN_STAGE_PIL_RESCALE, IRN_STAGE_TV_RESIZE = 0, 1, 2


def irn_reduced_size(S):
    """the side of imutils.pil_rescale(label, 0.25, 0) of an S x S crop"""
    return int(np.round(int(S) * 0.25))


def irn_train_batch(ctx, images_dev, labels_dev, sizes, image_offsets, label_offsets, params, S, mean, std, pre_div255, stage, x_dev,
                    label_dev, reduced_dev):
    """wsc_irn_train_batch: packed decoded images ([H][W][3] at byte `image_offsets`) and IR labels ([H][W] at byte
    `label_offsets`) -> x_dev float32 [B][3][S][S], label_dev uint8 [B][S][S], reduced_dev uint8 [B][s][s] (irn_reduced_size).
    params: integer (B, 9) records in the order of IRN_BATCH_PARAMS.  Shapes and dtypes are checked here, before any C call; the
    windows by the library."""
    B = len(sizes)
    if not 1 <= B <= 65535:
        raise ValueError("irn_train_batch: %d samples (1 .. 65535)" % B)
    size_hw = _hw_table("irn_train_batch: sizes", sizes, B)
    ioff = _offset_table("irn_train_batch: image_offsets", image_offsets, B)
    loff = _offset_table("irn_train_batch: label_offsets", label_offsets, B)
    p = np.asarray(params)
    if p.shape != (B, len(IRN_BATCH_PARAMS)) or p.dtype.kind not in "iu":
        raise ValueError("irn_train_batch: params %r %s, expected integer (%d, %d)" % (p.shape, p.dtype, B, len(IRN_BATCH_PARAMS)))
    p = np.ascontiguousarray(p, dtype=np.int32)
    m, sd = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    if m.shape != (3,) or sd.shape != (3,) or not np.isfinite(m).all() or not np.isfinite(sd).all() or (sd == 0).any():
        raise ValueError("irn_train_batch: mean %r / std %r, expected three finite values each and no zero std" % (m.shape, sd.shape))
    m, sd = np.ascontiguousarray(m), np.ascontiguousarray(sd)
    if int(S) != S or not 2 <= int(S) <= 8192:
        raise ValueError("irn_train_batch: S = %r (2 .. 8192)" % (S,))
    check(ctx._lib.wsc_irn_train_batch(ctx.h, _ptr(images_dev), _ptr(labels_dev), B, size_hw.ctypes.data, ioff.ctypes.data,
                                       loff.ctypes.data, p.ctypes.data, int(S), m.ctypes.data, sd.ctypes.data, int(bool(pre_div255)),
                                       int(stage), _ptr(x_dev), _ptr(label_dev), _ptr(reduced_dev)))


CLS_FILL_MODES = {"nearest": 0, "reflect": 1, "constant": 2}  # WSC_CLS_FILL_*
CLS_FLAG_WARP, CLS_FLAG_FLIP_COLS, CLS_FLAG_FLIP_ROWS = 1, 2, 4  # WSC_CLS_FLAG_*


def cls_train_batch(ctx, images_dev, sizes, offsets, hw, affine, flags, fill_mode, cval, sub3, div, mul, x_dev):
    """wsc_cls_train_batch: packed decoded RGB images ([H_b][W_b][3] at byte `offsets`) -> x_dev float32 [B][3][H][W]: PIL nearest
    resize to hw = (H, W), scipy's order-1 affine warp where bit 0 of a sample's flags is set, the flips (bits 1, 2), ((v - sub[c])
    / div) * mul.  affine: (B, 6) float64 rows M00 M01 M10 M11 off0 off1 (axis 0 the row); flags: B integers; fill_mode: 'nearest' /
    'reflect' / 'constant' or its number.  Shapes and dtypes are checked here, before any C call; the values by the library."""
    B = len(sizes)
    if not 1 <= B <= 65535:
        raise ValueError("cls_train_batch: %d samples (1 .. 65535)" % B)
    size_hw = _hw_table("cls_train_batch: sizes", sizes, B)
    off = _offset_table("cls_train_batch: offsets", offsets, B)
    a = np.asarray(affine)
    if a.shape != (B, 6) or a.dtype.kind != "f":
        raise ValueError("cls_train_batch: affine %r %s, expected float (%d, 6)" % (a.shape, a.dtype, B))
    a = np.ascontiguousarray(a, dtype=np.float64)
    f = np.asarray(flags)
    if f.shape != (B,) or f.dtype.kind not in "iu":
        raise ValueError("cls_train_batch: flags %r %s, expected %d integers" % (f.shape, f.dtype, B))
    f = np.ascontiguousarray(f, dtype=np.int32)
    s = np.ascontiguousarray(sub3, dtype=np.float32)
    if s.shape != (3,):
        raise ValueError("cls_train_batch: sub3 has shape %r, expected (3,)" % (s.shape,))
    if isinstance(fill_mode, str):
        if fill_mode not in CLS_FILL_MODES:
            raise ValueError("cls_train_batch: fill_mode %r (one of %s)" % (fill_mode, sorted(CLS_FILL_MODES)))
        fill_mode = CLS_FILL_MODES[fill_mode]
    H, W = int(hw[0]), int(hw[1])
    check(ctx._lib.wsc_cls_train_batch(ctx.h, _ptr(images_dev), B, size_hw.ctypes.data, off.ctypes.data, H, W, a.ctypes.data,
                                       f.ctypes.data, int(fill_mode), float(cval), s.ctypes.data, float(div), float(mul), _ptr(x_dev)))


def label_unary_from_cam(ctx, highres_dev, B, K, N, thres, gt_prob, unary_dev, labels_dev=None):
    check(ctx._lib.wsc_label_unary_from_cam(ctx.h, _ptr(highres_dev), B, K, N, float(thres), float(gt_prob), _ptr(unary_dev),
                                            _ptr(labels_dev)))


def dsrg_seed_grow(ctx, tags_dev, cues_dev, probs_dev, B, H, W, C, out_dev, th_f=0.5, th_b=0.7):
    """wsc_dsrg_seed_grow: DSRG seeded region growing of a batch (NHWC float32); out_dev may be cues_dev."""
    check(ctx._lib.wsc_dsrg_seed_grow(ctx.h, _ptr(tags_dev), _ptr(cues_dev), _ptr(probs_dev), int(B), int(H), int(W), int(C),
                                      float(th_f), float(th_b), _ptr(out_dev)))


SEG_LOSS_SEC, SEG_LOSS_DSRG = 0, 1
# slots of wsc_seg_loss's loss_dev (include/wsscam.h WSC_SEG_LOSS_*), under the reference's names
SEG_LOSS_SLOTS = ("seed", "constrain", "expand", "loss_1", "loss_2", "loss_3", "norm", "seed_bg", "seed_fg")


def seg_loss(ctx, method, prob_dev, crf_dev, cues_dev, labels_dev, B, H, W, C, min_prob, w_fg, z_fg, w_bg, z_bg, loss_dev,
             grad_prob_dev=None, grad_fc8_dev=None):
    """wsc_seg_loss: the SEC / DSRG losses (float64 [len(SEG_LOSS_SLOTS)] in loss_dev) and, where a buffer is given, d norm / d p and
    d norm / d fc8 (float32 NHWC).  w_fg / w_bg: float32 host tables [H * W] (SEC; None for DSRG); asynchronous."""
    tabs = []
    for w in (w_fg, w_bg):
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (int(H) * int(W),):
                raise ValueError("seg_loss: a weight table of shape %r for %d x %d maps" % (w.shape, H, W))
        tabs.append(w)
    check(ctx._lib.wsc_seg_loss(ctx.h, int(method), _ptr(prob_dev), _ptr(crf_dev), _ptr(cues_dev), _ptr(labels_dev), int(B), int(H),
                                int(W), int(C), float(min_prob), _ptr(tabs[0]), float(z_fg), _ptr(tabs[1]), float(z_bg),
                                _ptr(loss_dev), _ptr(grad_prob_dev), _ptr(grad_fc8_dev)))


# slots of wsc_irn_aff_loss's loss_dev (include/wsscam.h WSC_IRN_LOSS_*)
IRN_LOSS_SLOTS = ("pos_bg", "pos_fg", "pos", "neg", "dp_fg", "dp_bg", "total", "n_bg", "n_fg", "n_neg")


def irn_aff_loss(ctx, edge_dev, dp_dev, label_dev, B, h, w, dirs, path_start, path_yx, radius_floor, valid_below, loss_dev,
                 grad_edge_dev=None, grad_dp_dev=None):
    """wsc_irn_aff_loss: the IRNet training loss (float64 [len(IRN_LOSS_SLOTS)] in loss_dev) of edge_dev float32 [B][h][w] (logits),
    dp_dev float32 [B][2][h][w] and label_dev uint8 [B][h][w] and, where a buffer is given, d total / d edge and d total / d dp.
    dirs / path_start / path_yx: PathIndex.device_tables(); asynchronous."""
    dirs = np.ascontiguousarray(dirs, dtype=np.int32)
    path_start = np.ascontiguousarray(path_start, dtype=np.int32)
    path_yx = np.ascontiguousarray(path_yx, dtype=np.int32)
    if dirs.ndim != 2 or dirs.shape[1] != 2 or path_start.shape != (dirs.shape[0] + 1,) or path_yx.ndim != 2 or path_yx.shape[1] != 2 \
            or (len(path_start) and int(path_start.max()) > path_yx.shape[0]):
        raise ValueError("irn_aff_loss: path tables of shapes %r, %r, %r" % (dirs.shape, path_start.shape, path_yx.shape))
    check(ctx._lib.wsc_irn_aff_loss(ctx.h, _ptr(edge_dev), _ptr(dp_dev), _ptr(label_dev), int(B), int(h), int(w), _ptr(dirs),
                                    _ptr(path_start), _ptr(path_yx), int(dirs.shape[0]), int(radius_floor), int(valid_below),
                                    _ptr(loss_dev), _ptr(grad_edge_dev), _ptr(grad_dp_dev)))


CLS_POOL_MEAN, CLS_POOL_MAX = 0, 1
# slots of wsc_cls_loss's loss_dev (include/wsscam.h WSC_CLS_LOSS_*)
CLS_LOSS_SLOTS = ("loss", "mean_loss", "n_equal", "tp", "possible", "predicted")
ROC_NO_POSITIVE, ROC_NO_NEGATIVE = 1, 2
# columns of wsc_cls_threshold_counts's counts_dev (WSC_CLS_COUNT_*)
CLS_COUNT_SLOTS = ("tp", "fp", "tn", "fn", "equal")


def cls_loss(ctx, feat_dev, B, n, F, pool, w_dev, bias_dev, C, target_dev, sample_weight, loss_dev, score_dev=None, grad_feat_dev=None,
             grad_w_dev=None, grad_bias_dev=None):
    """wsc_cls_loss: binary cross-entropy and the metric counts of the classifier head (float64 [len(CLS_LOSS_SLOTS)] in loss_dev) on
    feat_dev float32 [B][n][F], w_dev [C][F], bias_dev [C] or None, target_dev [B][C]; sample_weight: host float32 [B] or None; where
    a buffer is given, the scores [B][C] and the gradients of the loss (feat [B][n][F], w [C][F], bias [C]); asynchronous."""
    sw = None
    if sample_weight is not None:
        sw = np.ascontiguousarray(sample_weight, dtype=np.float32)
        if sw.shape != (int(B),):
            raise ValueError("cls_loss: sample_weight of shape %r for %d samples" % (sw.shape, B))
    check(ctx._lib.wsc_cls_loss(ctx.h, _ptr(feat_dev), int(B), int(n), int(F), int(pool), _ptr(w_dev), _ptr(bias_dev), int(C),
                                _ptr(target_dev), _ptr(sw), _ptr(loss_dev), _ptr(score_dev), _ptr(grad_feat_dev), _ptr(grad_w_dev),
                                _ptr(grad_bias_dev)))


def roc_thresholds(ctx, score_dev, target_dev, N, C, thresh_dev, status_dev, n_points_dev=None, fps_dev=None, tps_dev=None):
    """wsc_roc_thresholds: per class the roc_curve threshold at the first minimum of |tpr - (1 - fpr)| (float32 [C]) and the status
    bits (int32 [C]) of score_dev / target_dev float32 [N][C]; optionally the kept curve, n_points int32 [C] and fps / tps int32
    [C][N + 1]; asynchronous."""
    check(ctx._lib.wsc_roc_thresholds(ctx.h, _ptr(score_dev), _ptr(target_dev), int(N), int(C), _ptr(thresh_dev), _ptr(status_dev),
                                      _ptr(n_points_dev), _ptr(fps_dev), _ptr(tps_dev)))


def cls_threshold_counts(ctx, score_dev, target_dev, N, C, thresh_dev, counts_dev):
    """wsc_cls_threshold_counts: counts_dev int64 [C][len(CLS_COUNT_SLOTS)] of score_dev >= thresh_dev[c] against target_dev."""
    check(ctx._lib.wsc_cls_threshold_counts(ctx.h, _ptr(score_dev), _ptr(target_dev), int(N), int(C), _ptr(thresh_dev), _ptr(counts_dev)))


def cls_scores_append(ctx, src_dev, elems, dst_dev):
    """wsc_cls_scores_append: elems floats from src_dev to dst_dev, on the stream."""
    check(ctx._lib.wsc_cls_scores_append(ctx.h, _ptr(src_dev), int(elems), _ptr(dst_dev)))


def cue_maps(ctx, cams_nhwc_dev, B, h, w, C_all, chan, gate_dev, S, out_dev):
    """wsc_cue_maps: out[b][c] = bilinear(cams[b][:, :, chan[c]] * gate[b][c]) to S x S, float32 [B][len(chan)][S][S]."""
    ch = np.ascontiguousarray(chan, dtype=np.int32)
    check(ctx._lib.wsc_cue_maps(ctx.h, _ptr(cams_nhwc_dev), int(B), int(h), int(w), int(C_all), ch.ctypes.data, len(ch),
                                _ptr(gate_dev), int(S), _ptr(out_dev)))


def cue_seeds(ctx, fg_dev, bg_dev, B, C, Cb, H, W, thresh, label_dev, area_dev=None, per_image_max=False, bg_fraction=0.1):
    """wsc_cue_seeds: float32 [B][C][H][W] foreground (+ [B][Cb][H][W] background, or None) stacks -> uint8 [B][H*W] seed labels
    (0 = none, k + 1 = localization channel k) and, with area_dev, int32 [B][L] mask areas."""
    check(ctx._lib.wsc_cue_seeds(ctx.h, _ptr(fg_dev), _ptr(bg_dev), int(B), int(C), int(Cb), int(H), int(W), float(thresh),
                                 int(bool(per_image_max)), float(bg_fraction), _ptr(label_dev), _ptr(area_dev)))


def _seg_tables(src_sizes, out_sizes, src_off, dst_off):
    B = len(src_sizes)
    return (B, np.ascontiguousarray(src_off, dtype=np.int64), _size_table(src_sizes, B), _size_table(out_sizes, B),
            np.ascontiguousarray(dst_off, dtype=np.int64))


def seg_unary_nhwc(ctx, prob_dev, C, src_sizes, out_sizes, prob_off, unary_off, unary_dev):
    """wsc_seg_unary_nhwc: packed NHWC softmax blocks [h_b][w_b][C] (float offsets prob_off) -> class-major unaries
    -log(bilinear resize to out_sizes[b]), [C][H_b*W_b] at float offsets unary_off."""
    B, so, sh, oh, do = _seg_tables(src_sizes, out_sizes, prob_off, unary_off)
    check(ctx._lib.wsc_seg_unary_nhwc(ctx.h, _ptr(prob_dev), B, int(C), so.ctypes.data, sh.ctypes.data, oh.ctypes.data, do.ctypes.data,
                                      _ptr(unary_dev)))


def seg_resize_argmax(ctx, q_dev, C, src_sizes, out_sizes, q_off, label_off, label_dev):
    """wsc_seg_resize_argmax: packed class-major marginals [C][h_b*w_b] (float offsets q_off) -> int32 labels, the first maximum
    over the classes of the bilinear resize to out_sizes[b], H_b*W_b per image at int32 offsets label_off."""
    B, so, sh, oh, do = _seg_tables(src_sizes, out_sizes, q_off, label_off)
    check(ctx._lib.wsc_seg_resize_argmax(ctx.h, _ptr(q_dev), B, int(C), so.ctypes.data, sh.ctypes.data, oh.ctypes.data, do.ctypes.data,
                                         _ptr(label_dev)))


def seg_preprocess_u8(ctx, img_dev, sizes, offsets, mean_bgr, out_hw, x_dev):
    """wsc_seg_preprocess_u8: packed uint8 RGB images ([h_i][w_i][3] blocks at byte `offsets`) -> float32 [n][H][W][3], the TF 1.x
    bilinear resize to out_hw, BGR, minus mean_bgr: image_preprocess of a ragged batch in one launch."""
    n = len(sizes)
    size_hw = _size_table(sizes, n)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    m = np.ascontiguousarray(mean_bgr, dtype=np.float32).reshape(3)
    check(ctx._lib.wsc_seg_preprocess_u8(ctx.h, _ptr(img_dev), n, size_hw.ctypes.data, off.ctypes.data, m.ctypes.data, int(out_hw[0]),
                                         int(out_hw[1]), _ptr(x_dev)))


def seg_crf_image_u8(ctx, x_dev, B, H, W, mean, out_hw, out_dev):
    """wsc_seg_crf_image_u8: float32 [B][H][W][3] -> uint8 [B][sh][sw][3], (x + mean) TF-resized to out_hw and cast as
    image.astype(np.uint8) (truncation to int32, low 8 bits): the CRF layer's zoomed image."""
    m = np.ascontiguousarray(mean, dtype=np.float32).reshape(3)
    check(ctx._lib.wsc_seg_crf_image_u8(ctx.h, _ptr(x_dev), int(B), int(H), int(W), m.ctypes.data, int(out_hw[0]), int(out_hw[1]),
                                        _ptr(out_dev)))


def seg_crf_logprob(ctx, q_dev, B, C, n, min_prob, out_dev):
    """wsc_seg_crf_logprob: class-major marginals [B][C][n] -> NHWC [B][n][C] log(clamp(q, min_prob) / their sum over the classes)."""
    check(ctx._lib.wsc_seg_crf_logprob(ctx.h, _ptr(q_dev), int(B), int(C), int(n), float(min_prob), _ptr(out_dev)))


def seg_planes_from_nhwc(ctx, src_dev, B, C, n, dst_dev):
    """wsc_seg_planes_from_nhwc: NHWC maps [B][n][C] -> class-major planes [B][C][n] (the layout seg_resize_argmax reads)."""
    check(ctx._lib.wsc_seg_planes_from_nhwc(ctx.h, _ptr(src_dev), int(B), int(C), int(n), _ptr(dst_dev)))


def seg_cue_tables(cues_per_sample, labels_per_sample):
    """The ragged host tables wsc_seg_train_batch takes -> (cues, cue_off, labels, label_off): cues_per_sample[b] the (3, n_b)
    (class, row, col) index lists of localization_cues.pickle (n_b = 0 is legal), labels_per_sample[b] the listed classes.
    cues: sample b's [3][n_b] int32 block at int index 3 * cue_off[b]; the offsets are int32 [B + 1]."""
    per = []
    for b, c in enumerate(cues_per_sample):
        c = np.asarray(c)
        if c.size and (c.ndim != 2 or c.shape[0] != 3 or c.dtype.kind not in "iu"):
            raise ValueError("seg_cue_tables: sample %d: cues %r %s, expected integer (3, n)" % (b, c.shape, c.dtype))
        per.append(c.reshape(-1))
    cues, off3 = _key_table(per)
    labels, label_off = _key_table(labels_per_sample)
    return cues, off3 // 3, labels, label_off


def seg_train_batch(ctx, img_dev, sizes, offsets, cues, cue_off, labels, label_off, mean_bgr, out_hw, s, C, x_dev, cues_dev, labels_dev):
    """wsc_seg_train_batch: packed uint8 RGB images (as seg_preprocess_u8 takes them) and the tables of seg_cue_tables ->
    x_dev float32 [B][H][W][3] (seg_preprocess_u8's bits), cues_dev float32 [B][s][s][C] (1.0 at the listed (row, col, class)),
    labels_dev float32 [B][C] (1.0 at the listed classes and at class 0).  The library checks every entry before any launch."""
    B = len(sizes)
    size_hw = _size_table(sizes, B)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    tabs = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in (cues, cue_off, labels, label_off)]
    if off.shape != (B,) or tabs[1].shape != (B + 1,) or tabs[3].shape != (B + 1,):
        raise ValueError("seg_train_batch: %d images, %r byte offsets, %r cue offsets, %r label offsets"
                         % (B, off.shape, tabs[1].shape, tabs[3].shape))
    m = np.ascontiguousarray(mean_bgr, dtype=np.float32).reshape(3)
    check(ctx._lib.wsc_seg_train_batch(ctx.h, _ptr(img_dev), B, size_hw.ctypes.data, off.ctypes.data, tabs[0].ctypes.data,
                                       tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data, m.ctypes.data, int(out_hw[0]),
                                       int(out_hw[1]), int(s), int(C), _ptr(x_dev), _ptr(cues_dev), _ptr(labels_dev)))


def seg_gt_index_tf(ctx, gt_dev, sizes, offsets, channels, colours, n_class, out_hw, index_dev):
    """wsc_seg_gt_index_tf: packed uint8 ground truths ([h_b][w_b][channels] blocks at byte `offsets`) -> uint8 [B][OH][OW] class
    indices in [0, n_class]: the TF 1.x nearest-neighbour resize (float32 index), then channel 0's value (colours None) or the
    first matching row of the uint8 (n_class, 3) colour table; no match: n_class."""
    B = len(sizes)
    size_hw = _size_table(sizes, B)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    if off.shape != (B,):
        raise ValueError("seg_gt_index_tf: %d ground truths, %r byte offsets" % (B, off.shape))
    col = None
    if colours is not None:
        col = np.ascontiguousarray(colours, dtype=np.uint8)
        if col.shape != (int(n_class), 3):
            raise ValueError("seg_gt_index_tf: colours %r for %d classes" % (col.shape, n_class))
    check(ctx._lib.wsc_seg_gt_index_tf(ctx.h, _ptr(gt_dev), B, size_hw.ctypes.data, off.ctypes.data, int(channels),
                                       None if col is None else col.ctypes.data, int(n_class), int(out_hw[0]), int(out_hw[1]),
                                       _ptr(index_dev)))


def ir_label_combine(ctx, fg_pred_dev, bg_pred_dev, keys, N, conf_dev):
    k = np.ascontiguousarray(keys, dtype=np.int32)
    B, M = k.shape
    check(ctx._lib.wsc_ir_label_combine(ctx.h, _ptr(fg_pred_dev), _ptr(bg_pred_dev), k.ctypes.data, B, M, N, _ptr(conf_dev)))
