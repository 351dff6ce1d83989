"""ctypes binding of the HIP column-DP core (include/instance_stixels_core.h).

This is the product path: it loads instance_stixels_amd/lib/libis_core.so and fails loudly if the
library is missing -- there is no CPU fallback.  PyTorch is used only as the owner of device
memory / streams (plumbing); every compute call goes through the C ABI.
"""
import ctypes
import functools
import math
import os

import numpy as np

from .config import StixelParams, SECTION_DTYPE, INSTANCE_CLASSES
from .evaluation import CITYSCAPES_N_LABELS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IS_CORE_LIB", os.path.join(_HERE, "lib", "libis_core.so"))
_LIB = None
EVAL_COUNTERS = 200   # IS_EVAL_COUNTERS of include/instance_stixels_core.h (checked by tests/test_host_and_abi.py)

EXPORTS = [
    "is_ctx_create", "is_ctx_destroy", "is_join_columns", "is_compute", "is_device_malloc",
    "is_device_free", "is_memcpy_h2d", "is_memcpy_d2h", "is_memcpy2d_d2h", "is_memset", "is_stream_synchronize",
    "is_device_synchronize", "is_last_error", "is_version", "is_set_kernel_timing",
    "is_get_kernel_times_ms", "is_scratch_bytes", "is_flip_and_pad", "is_road_vdisparity",
    "is_cluster_instances", "is_host_malloc", "is_host_free", "is_get_device", "is_set_device",
    "is_ctx_device", "is_set_eval_counters", "is_get_eval_counters",
    "is_pack_sections", "is_unpack_sections", "is_stream_create", "is_stream_destroy",
    "is_debug_read_object_lut", "is_debug_read_block_summaries", "is_debug_lut_fused_state",
    "is_lut_fused_repairs", "is_debug_unary_path", "is_debug_read_lut_carries", "is_debug_lut_carry_lds",
    "is_comm_unique_id", "is_comm_init_rank", "is_comm_destroy", "is_comm_rank", "is_gather_i32",
    "is_gather_sections",
    "is_road_ctx_create", "is_road_ctx_destroy", "is_road_ctx_device", "is_road_ctx_binary",
    "is_road_choose_batch", "is_ctx_set_ground_model", "is_compute_road", "is_debug_read_ground",
    "is_road_vdisparity_batch", "is_road_hough_batch",
    "is_section_instance_labels", "is_render_sections",
    "is_instance_overlap", "is_pack_overlap_records",
    "is_stixel_world",
    "is_assign_instances_gt", "is_pack_section_labels",
    "is_instance_objects",
    "is_compute_sweep", "is_recluster",
    "is_cluster_instance_disparity", "is_instance_disparity_scratch_bytes",
    "is_mode_downsample", "is_gt_targets_scratch_bytes", "is_gt_instance_targets",
    "is_offset_loss_scratch_bytes", "is_offset_loss",
    "is_segmentation_head",
    "is_segmentation_head_backward_scratch_bytes", "is_segmentation_head_backward",
    "is_semantic_nll_scratch_bytes", "is_semantic_nll",
    "is_cnn_label_maps",
    "is_semantic_nll_up_scratch_bytes", "is_semantic_nll_up",
    "is_conv3x3_packed_bytes", "is_conv3x3_pack_weights", "is_conv3x3_bn_relu",
    "is_conv_packed_bytes", "is_conv_pack_weights", "is_conv_bn",
    "is_conv_bn_stride",
    "is_stem_packed_bytes", "is_stem_pack_weights", "is_stem",
    "is_conv_bn_backward_scratch_bytes", "is_conv_bn_backward",
    "is_conv_bn_stride_backward_scratch_bytes", "is_conv_bn_stride_backward",
    "is_stem_backward_scratch_bytes", "is_stem_backward", "is_stem_backward_constant",
]
RENDER_MAX_LABELS = 64    # IS_RENDER_MAX_LABELS
RENDER_MAX_CLASSES = 256  # IS_RENDER_MAX_CLASSES
OVERLAP_MAX_CAPACITY = 1 << 28  # IS_OVERLAP_MAX_CAPACITY
# is_overlap_record: one entry of a frame's joint histogram of instance image and gt instanceIds
OVERLAP_DTYPE = np.dtype([("pred", np.int32), ("gt", np.int32), ("count", np.int64)])


class InstanceBuffers(ctypes.Structure):
    _fields_ = [("d_centerofmass", ctypes.c_void_p), ("d_indices", ctypes.c_void_p),
                ("d_core_candidates", ctypes.c_void_p), ("d_instances_per_class", ctypes.c_void_p),
                ("d_labels", ctypes.c_void_p), ("d_packed", ctypes.c_void_p)]


class SweepSet(ctypes.Structure):
    """is_sweep_set: the seven parameters one set of a sweep changes (instance_weight relative to
    segmentation_weight, as in StixelParams); 32 bytes."""
    _fields_ = [("prior_weight", ctypes.c_float), ("disparity_weight", ctypes.c_float),
                ("segmentation_weight", ctypes.c_float), ("instance_weight", ctypes.c_float),
                ("clustering_eps", ctypes.c_float), ("clustering_min_pts", ctypes.c_int),
                ("clustering_size_filter", ctypes.c_int), ("reserved", ctypes.c_int)]


class RenderArgs(ctypes.Structure):
    """is_render_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_sections", vp), ("d_section_instance", vp), ("n_images", ci), ("realcols", ci),
                ("max_sections", ci), ("rows", ci), ("cols", ci), ("h_class_to_label", vp), ("n_classes", ci),
                ("d_label", vp), ("d_disparity", vp), ("d_instance", vp), ("d_gt_label", vp), ("n_labels", ci),
                ("d_confusion", vp), ("d_gt_disparity", vp), ("d_disp_abs_sum", vp), ("d_disp_count", vp),
                ("d_stixel_count", vp)]


class InstanceOverlapArgs(ctypes.Structure):
    """is_instance_overlap_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_sections", vp), ("d_section_instance", vp), ("n_images", ci), ("realcols", ci),
                ("max_sections", ci), ("rows", ci), ("cols", ci), ("d_gt_instance", vp), ("capacity", ci),
                ("d_records", vp), ("d_n_records", vp), ("d_overflow", vp)]


# is_world_stixel: one stixel of the 3-D world of a frame (is_stixel_world, Stixels::WorldBatch), 96 bytes
WORLD_DTYPE = np.dtype([
    ("column", np.int32), ("section", np.int32), ("type", np.int32), ("vB", np.int32), ("vT", np.int32),
    ("semantic_class", np.int32), ("instance_id", np.int32), ("disparity", np.float32), ("cost", np.float32),
    ("instance_meanx", np.float32), ("instance_meany", np.float32), ("vertices", np.float32, (12,)),
    ("reserved", np.int32),
])
assert WORLD_DTYPE.itemsize == 96


class WorldStixel(ctypes.Structure):
    """is_world_stixel, for the layout checks of the tests."""
    _fields_ = [("column", ctypes.c_int32), ("section", ctypes.c_int32), ("type", ctypes.c_int32),
                ("vB", ctypes.c_int32), ("vT", ctypes.c_int32), ("semantic_class", ctypes.c_int32),
                ("instance_id", ctypes.c_int32), ("disparity", ctypes.c_float), ("cost", ctypes.c_float),
                ("instance_meanx", ctypes.c_float), ("instance_meany", ctypes.c_float),
                ("vertices", ctypes.c_float * 12), ("reserved", ctypes.c_int32)]


class WorldArgs(ctypes.Structure):
    """is_world_args: zero-initialised by ctypes; device pointers as ints, h_* host pointers."""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("d_sections", vp), ("d_section_instance", vp), ("n_images", ci), ("realcols", ci),
                ("max_sections", ci), ("rows", ci), ("column_step", ci), ("focal", cf), ("baseline", cf),
                ("camera_center_x", cf), ("camera_center_y", cf), ("h_alpha_ground", vp), ("h_vhor", vp),
                ("capacity", ci), ("d_counts", vp), ("d_offsets", vp), ("d_frame_totals", vp), ("d_world", vp)]


class AssignGtArgs(ctypes.Structure):
    """is_assign_gt_args: zero-initialised by ctypes; device pointers as ints, h_label_ids a host pointer."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_sections", vp), ("d_gt_instance", vp), ("n_images", ci), ("rows", ci), ("cols", ci),
                ("realcols", ci), ("max_sections", ci), ("min_fraction", ctypes.c_double), ("h_label_ids", vp),
                ("gt_is_train_ids", ci), ("d_section_instance", vp), ("d_section_votes", vp)]


# is_instance_object: one instance of a frame (is_instance_objects, Stixels::InstanceObjectsBatch), 64 bytes
OBJECT_DTYPE = np.dtype([
    ("frame", np.int32), ("semantic_class", np.int32), ("label", np.int32), ("n_stixels", np.int32),
    ("n_columns", np.int32), ("first_point", np.int32), ("pixels", np.int32), ("col_min", np.int32),
    ("col_max", np.int32), ("top", np.int32), ("bottom", np.int32), ("reserved", np.int32),
    ("disparity_min", np.float32), ("disparity_max", np.float32), ("disparity_q16_sum", np.int64),
])
# is_contour_point: the depth-closest stixel of an object in one stixel column, 32 bytes
CONTOUR_DTYPE = np.dtype([
    ("object", np.int32), ("column", np.int32), ("section", np.int32), ("vB", np.int32),
    ("vT", np.int32), ("column_pixels", np.int32), ("disparity", np.float32), ("reserved", np.int32),
])
assert OBJECT_DTYPE.itemsize == 64 and CONTOUR_DTYPE.itemsize == 32


class InstanceObjectsArgs(ctypes.Structure):
    """is_instance_objects_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_sections", vp), ("d_section_instance", vp), ("n_images", ci), ("realcols", ci),
                ("max_sections", ci), ("rows", ci), ("cols", ci), ("object_capacity", ci), ("point_capacity", ci),
                ("d_objects", vp), ("d_points", vp), ("d_frame_objects", vp), ("d_frame_points", vp),
                ("d_totals", vp)]


INSTANCE_DISPARITY_KEYS = 8000  # IS_INSTANCE_DISPARITY_KEYS


class InstanceDisparityArgs(ctypes.Structure):
    """is_instance_disparity_args: zero-initialised by ctypes; device pointers as ints, instances a host pointer."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_sections", vp), ("d_gt_instance", vp), ("d_disparity_u8", vp), ("n_images", ci), ("rows", ci),
                ("cols", ci), ("realcols", ci), ("max_sections", ci), ("instances", vp), ("eps", ctypes.c_float),
                ("min_pts", ci), ("size_filter", ci), ("capacity", ci), ("d_scratch", vp),
                ("scratch_bytes", ctypes.c_size_t), ("d_stixel_median", vp), ("d_key_count", vp), ("d_key_median", vp)]


GT_TARGETS_MAX_CAPACITY = 8192  # IS_GT_TARGETS_MAX_CAPACITY
DTYPE_UINT8, DTYPE_UINT16, DTYPE_INT32 = 0, 1, 2  # IS_DTYPE_*


class GtTargetsArgs(ctypes.Structure):
    """is_gt_targets_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_gt_instance", vp), ("d_disparity_u16", vp), ("n_images", ci), ("rows", ci), ("cols", ci),
                ("d_targets", vp), ("target_planes", ci), ("d_ids8", vp), ("d_segmentation", vp),
                ("rows_power2_segmentation", ci), ("channels", ci), ("capacity", ci), ("d_scratch", vp),
                ("scratch_bytes", ctypes.c_size_t), ("d_key_count", vp)]


class OffsetLossArgs(ctypes.Structure):
    """is_offset_loss_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    _fields_ = [("d_prediction", vp), ("prediction_image_stride", ll), ("d_ids8", vp), ("d_disparity8_u16", vp),
                ("n_images", ci), ("planes", ci), ("rows8", ci), ("cols8", ci), ("w_offset_mean", cf),
                ("w_offset_variance", cf), ("w_disparity_mean", cf), ("w_disparity_variance", cf),
                ("abs_variance", ci), ("d_loss", vp), ("d_terms", vp), ("d_grad", vp), ("grad_image_stride", ll),
                ("capacity", ci), ("d_scratch", vp), ("scratch_bytes", ctypes.c_size_t), ("d_key_count", vp)]


HEAD_MAX_CHANNELS = 32  # IS_HEAD_MAX_CHANNELS
HEAD_F32, HEAD_F16, HEAD_BF16 = 0, 1, 2  # IS_HEAD_*


class SegmentationHeadArgs(ctypes.Structure):
    """is_segmentation_head_args: zero-initialised by ctypes (set clamp_channel = -1 for no clamp); device pointers
    as ints."""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("K", ci), ("rows8", ci), ("cols8", ci),
                ("d_weight", vp), ("d_bias", vp), ("n_classes", ci), ("n_regression", ci),
                ("rows_power2_segmentation", ci), ("clamp_channel", ci), ("clamp_lo", cf), ("clamp_hi", cf),
                ("d_cnn_out", vp), ("d_segmentation", vp), ("reserved", ci * 4)]


HEAD_BACKWARD_CHUNK = 2048  # IS_HEAD_BACKWARD_CHUNK


class SegmentationHeadBackwardArgs(ctypes.Structure):
    """is_segmentation_head_backward_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("K", ci), ("rows8", ci), ("cols8", ci),
                ("d_weight", vp), ("n_classes", ci), ("n_regression", ci), ("d_cnn_out", vp), ("d_grad_out", vp),
                ("grad_image_stride", ll), ("d_grad_features", vp), ("d_grad_weight", vp), ("d_grad_bias", vp),
                ("d_grad_logits", vp), ("d_scratch", vp), ("scratch_bytes", ctypes.c_size_t), ("reserved", ci * 4)]


class SemanticNllArgs(ctypes.Structure):
    """is_semantic_nll_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("d_cnn_out", vp), ("cnn_image_stride", ll), ("d_target", vp), ("target_dtype", ci),
                ("ignore_index", ci), ("n_images", ci), ("rows8", ci), ("cols8", ci), ("n_classes", ci),
                ("d_loss", vp), ("d_valid_count", vp), ("d_bad_count", vp), ("d_grad", vp),
                ("grad_image_stride", ll), ("d_scratch", vp), ("scratch_bytes", ctypes.c_size_t),
                ("reserved", ci * 4)]


CNN_UP_NEAREST, CNN_UP_DECONV = 0, 1  # IS_CNN_UP_*
CNN_UP_MODES = {"nearest": CNN_UP_NEAREST, "deconv": CNN_UP_DECONV}


class CnnLabelArgs(ctypes.Structure):
    """is_cnn_label_args: zero-initialised by ctypes; device pointers as ints, h_class_to_label a host pointer."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_cnn_out", vp), ("n_images", ci), ("channels", ci), ("n_classes", ci), ("rows8", ci), ("cols8", ci),
                ("mode", ci), ("rows", ci), ("cols", ci), ("h_class_to_label", vp), ("d_class8", vp), ("d_label", vp),
                ("d_gt_label", vp), ("n_labels", ci), ("d_confusion", vp), ("reserved", ci * 4)]


class SemanticNllUpArgs(ctypes.Structure):
    """is_semantic_nll_up_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("d_cnn_out", vp), ("cnn_image_stride", ll), ("d_target", vp), ("ignore_index", ci),
                ("n_images", ci), ("rows8", ci), ("cols8", ci), ("n_classes", ci), ("mode", ci), ("rows", ci),
                ("cols", ci), ("d_loss", vp), ("d_valid_count", vp), ("d_bad_count", vp), ("d_grad", vp),
                ("grad_image_stride", ll), ("d_scratch", vp), ("scratch_bytes", ctypes.c_size_t),
                ("reserved", ci * 4)]


class Conv3x3Args(ctypes.Structure):
    """is_conv3x3_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("channels_in", ci), ("channels_out", ci),
                ("rows8", ci), ("cols8", ci), ("dilation", ci), ("d_packed", vp), ("d_scale", vp), ("d_shift", vp),
                ("relu", ci), ("d_out", vp), ("out_dtype", ci), ("reserved", ci * 4)]


class ConvBnArgs(ctypes.Structure):
    """is_conv_bn_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("channels_in", ci), ("channels_out", ci),
                ("rows8", ci), ("cols8", ci), ("kernel", ci), ("dilation", ci), ("d_packed", vp), ("d_scale", vp),
                ("d_shift", vp), ("d_residual", vp), ("relu", ci), ("d_out", vp), ("out_dtype", ci),
                ("reserved", ci * 4)]


class ConvBnStrideArgs(ctypes.Structure):
    """is_conv_bn_stride_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("channels_in", ci), ("channels_out", ci),
                ("rows_in", ci), ("cols_in", ci), ("kernel", ci), ("stride", ci), ("dilation", ci), ("d_packed", vp),
                ("d_scale", vp), ("d_shift", vp), ("d_residual", vp), ("relu", ci), ("d_out", vp), ("out_dtype", ci),
                ("reserved", ci * 4)]


class StemArgs(ctypes.Structure):
    """is_stem_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("d_image", vp), ("n_images", ci), ("rows", ci), ("cols", ci), ("d_lut", vp), ("dtype", ci),
                ("d_packed", vp), ("d_scale0", vp), ("d_shift0", vp), ("d_scale1", vp), ("d_shift1", vp), ("d_mid", vp),
                ("d_out", vp), ("reserved", ci * 4)]


CONV_BACKWARD_BAND = 32  # IS_CONV_BACKWARD_BAND


class ConvBnBackwardArgs(ctypes.Structure):
    """is_conv_bn_backward_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("channels_in", ci), ("channels_out", ci),
                ("rows8", ci), ("cols8", ci), ("kernel", ci), ("dilation", ci), ("d_weight", vp), ("d_scale", vp),
                ("d_out", vp), ("out_dtype", ci), ("relu", ci), ("d_grad_out", vp), ("grad_out_dtype", ci),
                ("grad_image_stride", ll), ("d_grad_features", vp), ("grad_features_dtype", ci),
                ("d_grad_features_add", vp), ("d_grad_weight", vp), ("d_grad_scale", vp), ("d_grad_shift", vp),
                ("d_grad_pre", vp), ("d_scratch", vp), ("scratch_bytes", ctypes.c_size_t), ("reserved", ci * 4)]


CONV_BACKWARD_STRIDE_BAND = 8  # IS_CONV_BACKWARD_STRIDE_BAND


class ConvBnStrideBackwardArgs(ctypes.Structure):
    """is_conv_bn_stride_backward_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("d_features", vp), ("dtype", ci), ("n_images", ci), ("channels_in", ci), ("channels_out", ci),
                ("rows_in", ci), ("cols_in", ci), ("kernel", ci), ("stride", ci), ("dilation", ci), ("d_weight", vp),
                ("d_scale", vp), ("d_out", vp), ("out_dtype", ci), ("relu", ci), ("d_grad_out", vp),
                ("grad_out_dtype", ci), ("grad_image_stride", ll), ("d_grad_features", vp),
                ("grad_features_dtype", ci), ("d_grad_features_add", vp), ("d_grad_weight", vp), ("d_grad_scale", vp),
                ("d_grad_shift", vp), ("d_grad_pre", vp), ("d_scratch", vp), ("scratch_bytes", ctypes.c_size_t),
                ("reserved", ci * 4)]


class StemBackwardArgs(ctypes.Structure):
    """is_stem_backward_args: zero-initialised by ctypes; device pointers as ints."""
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("d_image", vp), ("n_images", ci), ("rows", ci), ("cols", ci), ("d_lut", vp), ("dtype", ci),
                ("d_w0", vp), ("d_w1", vp), ("d_scale0", vp), ("d_scale1", vp), ("d_mid", vp), ("d_out", vp),
                ("d_grad_out", vp), ("grad_out_dtype", ci), ("grad_image_stride", ll), ("d_grad_next", vp),
                ("channels_next", ci), ("d_weight_next", vp), ("d_scale_next", vp), ("d_grad_weight0", vp),
                ("d_grad_scale0", vp), ("d_grad_shift0", vp), ("d_grad_weight1", vp), ("d_grad_scale1", vp),
                ("d_grad_shift1", vp), ("d_grad_pre1", vp), ("d_grad_pre0", vp), ("d_scratch", vp),
                ("scratch_bytes", ctypes.c_size_t), ("reserved", ci * 4)]


# IS_STEM_BACKWARD_BAND, _SEGMENT, _TILE_ROWS and _TILE_COLS, read from the library on first use (__getattr__ below)
_STEM_BACKWARD_CONSTANTS = {"STEM_BACKWARD_BAND": 0, "STEM_BACKWARD_SEGMENT": 1, "STEM_BACKWARD_TILE_ROWS": 2,
                            "STEM_BACKWARD_TILE_COLS": 3}


def __getattr__(name):
    if name in _STEM_BACKWARD_CONSTANTS:
        return int(lib().is_stem_backward_constant(_STEM_BACKWARD_CONSTANTS[name]))
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class RoadParams(ctypes.Structure):
    """is_road_params: one frame's road, the layout of Stixels::RoadParameters (16 bytes)"""
    _fields_ = [("vhor", ctypes.c_int), ("tilt", ctypes.c_float), ("height", ctypes.c_float),
                ("alpha", ctypes.c_float)]


class GroundParams(ctypes.Structure):
    """is_ground_params: the constants of the device ground model (is_ctx_set_ground_model)"""
    _fields_ = [(k, ctypes.c_float) for k in ("focal", "baseline", "max_dis", "pout", "sigma_disparity_ground",
                                              "sigma_camera_height", "sigma_camera_tilt")]


ROAD_DTYPE = np.dtype([("vhor", np.int32), ("tilt", np.float32), ("height", np.float32), ("alpha", np.float32)])
ROAD_NONE, ROAD_OK, ROAD_UNDECIDED, ROAD_HORIZON = 0, 1, 2, 3   # d_status of is_road_choose_batch


# The entry points of the C ABI with the signature (const X_args*, void* stream) and the class of X here: lib() sets
# their argtypes from this table, and _args_ptr makes the `_ptr` functions that only fill the struct.
_ARGS_ENTRY = {
    "is_render_sections": RenderArgs, "is_instance_overlap": InstanceOverlapArgs, "is_stixel_world": WorldArgs,
    "is_assign_instances_gt": AssignGtArgs, "is_instance_objects": InstanceObjectsArgs,
    "is_cluster_instance_disparity": InstanceDisparityArgs, "is_gt_instance_targets": GtTargetsArgs,
    "is_offset_loss": OffsetLossArgs, "is_segmentation_head": SegmentationHeadArgs,
    "is_segmentation_head_backward": SegmentationHeadBackwardArgs, "is_semantic_nll": SemanticNllArgs,
    "is_cnn_label_maps": CnnLabelArgs, "is_semantic_nll_up": SemanticNllUpArgs, "is_conv3x3_bn_relu": Conv3x3Args,
    "is_conv_bn": ConvBnArgs, "is_conv_bn_stride": ConvBnStrideArgs, "is_stem": StemArgs,
    "is_conv_bn_backward": ConvBnBackwardArgs, "is_conv_bn_stride_backward": ConvBnStrideBackwardArgs,
    "is_stem_backward": StemBackwardArgs,
}


class CoreError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise CoreError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7).  Two HIP
        # runtimes in one process do not work ("No HIP GPUs are available"), so when torch is
        # importable it must be loaded FIRST; the dynamic linker then resolves this library's
        # libamdhip64.so.7 dependency to the already loaded copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.is_ctx_create.argtypes = [ctypes.POINTER(StixelParams), vp, vp, ci, ci,
                                    ctypes.POINTER(vp)]
        L.is_ctx_destroy.argtypes = [vp]
        L.is_join_columns.argtypes = [vp, vp, ci, ci, vp, ci, vp]
        L.is_compute.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.is_device_malloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        L.is_device_free.argtypes = [vp]
        L.is_memcpy_h2d.argtypes = [vp, vp, ctypes.c_size_t, vp]
        L.is_memcpy_d2h.argtypes = [vp, vp, ctypes.c_size_t, vp]
        L.is_memcpy2d_d2h.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]
        L.is_memset.argtypes = [vp, ci, ctypes.c_size_t, vp]
        L.is_stream_synchronize.argtypes = [vp]
        L.is_last_error.restype = ctypes.c_char_p
        L.is_version.restype = ctypes.c_char_p
        L.is_set_kernel_timing.argtypes = [vp, ci]
        L.is_get_kernel_times_ms.argtypes = [vp, ctypes.POINTER(cf), ctypes.POINTER(cf),
                                             ctypes.POINTER(cf)]
        L.is_flip_and_pad.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp]
        L.is_road_vdisparity.argtypes = [vp, ci, ci, ci, cf, vp, vp, vp, vp]
        L.is_road_ctx_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, ci]
        L.is_road_ctx_destroy.argtypes = [vp]
        L.is_road_ctx_device.argtypes = [vp]
        L.is_road_ctx_binary.argtypes = [vp]
        L.is_road_ctx_binary.restype = vp
        L.is_road_vdisparity_batch.argtypes = [vp, vp, ci, cf, vp, vp, vp, vp]
        L.is_road_hough_batch.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.is_road_choose_batch.argtypes = [vp, ci, vp, vp, vp, ci, cf, cf, cf, cf, cf, RoadParams, vp, vp, vp]
        L.is_ctx_set_ground_model.argtypes = [vp, ctypes.POINTER(GroundParams), vp, ci]
        L.is_compute_road.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, vp]
        L.is_debug_read_ground.argtypes = [vp, ci, vp, ctypes.POINTER(ci)]
        for entry, args_cls in _ARGS_ENTRY.items():
            getattr(L, entry).argtypes = [ctypes.POINTER(args_cls), vp]
        L.is_cluster_instances.argtypes = [vp, ctypes.POINTER(InstanceBuffers), vp]
        L.is_section_instance_labels.argtypes = [ctypes.POINTER(InstanceBuffers), ci, ci, ci, vp, vp]
        L.is_pack_overlap_records.argtypes = [vp, vp, ci, ci, vp, vp]
        L.is_pack_section_labels.argtypes = [vp, ci, ci, ci, ci, vp, vp]
        L.is_compute_sweep.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp]
        L.is_recluster.argtypes = [vp, vp, ci, cf, ci, ci, vp, vp]
        L.is_instance_disparity_scratch_bytes.argtypes = [ci, ci, ci, ci]
        L.is_instance_disparity_scratch_bytes.restype = ctypes.c_size_t
        L.is_mode_downsample.argtypes = [vp, ci, ci, ci, ci, vp, vp]
        L.is_gt_targets_scratch_bytes.argtypes = [ci, ci, ci, ci, ci]
        L.is_gt_targets_scratch_bytes.restype = ctypes.c_size_t
        L.is_offset_loss_scratch_bytes.argtypes = [ci, ci, ci, ci, ci]
        L.is_offset_loss_scratch_bytes.restype = ctypes.c_size_t
        L.is_segmentation_head_backward_scratch_bytes.argtypes = [ci, ci, ci, ci, ci]
        L.is_segmentation_head_backward_scratch_bytes.restype = ctypes.c_size_t
        L.is_semantic_nll_scratch_bytes.argtypes = [ci, ci, ci]
        L.is_semantic_nll_scratch_bytes.restype = ctypes.c_size_t
        L.is_semantic_nll_up_scratch_bytes.argtypes = [ci, ci, ci, ci]
        L.is_semantic_nll_up_scratch_bytes.restype = ctypes.c_size_t
        L.is_conv3x3_packed_bytes.argtypes = [ci, ci, ci]
        L.is_conv3x3_packed_bytes.restype = ctypes.c_size_t
        L.is_conv3x3_pack_weights.argtypes = [vp, ci, ci, ci, vp, vp]
        L.is_conv_packed_bytes.argtypes = [ci, ci, ci, ci]
        L.is_conv_packed_bytes.restype = ctypes.c_size_t
        L.is_conv_pack_weights.argtypes = [vp, ci, ci, ci, ci, vp, vp]
        L.is_stem_packed_bytes.argtypes = [ci]
        L.is_stem_packed_bytes.restype = ctypes.c_size_t
        L.is_stem_pack_weights.argtypes = [vp, vp, ci, vp, vp]
        L.is_conv_bn_backward_scratch_bytes.argtypes = [ci, ci, ci, ci, ci, ci, ci]
        L.is_conv_bn_backward_scratch_bytes.restype = ctypes.c_size_t
        L.is_conv_bn_stride_backward_scratch_bytes.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci]
        L.is_conv_bn_stride_backward_scratch_bytes.restype = ctypes.c_size_t
        L.is_stem_backward_scratch_bytes.argtypes = [ci, ci, ci, ci, ci]
        L.is_stem_backward_scratch_bytes.restype = ctypes.c_size_t
        L.is_stem_backward_constant.argtypes = [ci]
        L.is_host_malloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        L.is_host_free.argtypes = [vp]
        L.is_get_device.argtypes = [ctypes.POINTER(ci)]
        L.is_set_device.argtypes = [ci]
        L.is_ctx_device.argtypes = [vp]
        L.is_set_eval_counters.argtypes = [vp, ci]
        L.is_get_eval_counters.argtypes = [vp, vp, ci]
        L.is_pack_sections.argtypes = [vp, ci, ci, vp, vp, vp, vp]
        L.is_unpack_sections.argtypes = [vp, vp, vp, ci, ci, vp, vp]
        L.is_scratch_bytes.argtypes = [vp]
        L.is_scratch_bytes.restype = ctypes.c_size_t
        L.is_comm_unique_id.argtypes = [vp, ctypes.c_size_t]
        L.is_comm_init_rank.argtypes = [ctypes.POINTER(vp), ci, vp, ci]
        L.is_comm_destroy.argtypes = [vp]
        L.is_comm_rank.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.is_gather_i32.argtypes = [vp, ci, vp, vp, vp, vp]
        L.is_gather_sections.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp, vp]
        L.is_debug_read_object_lut.argtypes = [vp, ci, vp]
        L.is_debug_lut_fused_state.argtypes = [vp, ctypes.POINTER(ci)]
        L.is_lut_fused_repairs.argtypes = [vp, ctypes.POINTER(ci)]
        L.is_debug_unary_path.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        try:   # (an experiment library built from an older tree may lack the newest test hooks)
            L.is_debug_read_block_summaries.argtypes = [vp, ci, vp, ci, ctypes.POINTER(ci)]
            L.is_debug_read_lut_carries.argtypes = [vp, ci, vp]
            L.is_debug_lut_carry_lds.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        except AttributeError:
            pass
        _LIB = L
    return _LIB


def _check(rc, what):
    if rc != 0:
        raise CoreError(f"{what} failed (rc={rc}): {lib().is_last_error().decode()}")


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Core:
    """One `is_ctx`: the device half of Stixels::Initialize .. Finish for a fixed configuration."""

    def __init__(self, params: StixelParams, obj_cost_lut, obj_disparity_range, max_batch=1,
                 device=0):
        self.params = StixelParams.from_buffer_copy(params)
        self.max_batch = int(max_batch)
        self.device = int(device)
        lut = np.ascontiguousarray(obj_cost_lut, np.float32)
        odr = np.ascontiguousarray(obj_disparity_range, np.float32)
        D = self.params.max_dis
        assert lut.size == D * D and odr.size == D
        self._ctx = ctypes.c_void_p()
        _check(lib().is_ctx_create(ctypes.byref(self.params), _hp(lut), _hp(odr), self.max_batch,
                                   self.device, ctypes.byref(self._ctx)), "is_ctx_create")

    def close(self):
        if self._ctx:
            lib().is_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def scratch_bytes(self):
        return int(lib().is_scratch_bytes(self._ctx))

    def set_kernel_timing(self, enabled=True):
        _check(lib().is_set_kernel_timing(self._ctx, int(enabled)), "is_set_kernel_timing")

    def set_eval_counters(self, enabled=True):
        """Evaluation counters of the branch-and-bound (never inside a timed region)."""
        _check(lib().is_set_eval_counters(self._ctx, int(enabled)), "is_set_eval_counters")

    def eval_counters(self):
        out = np.zeros(EVAL_COUNTERS, np.uint64)
        rc = lib().is_get_eval_counters(self._ctx, _hp(out), EVAL_COUNTERS)
        if rc != 0:   # (an experiment library built from an older tree only knows the first eight)
            _check(lib().is_get_eval_counters(self._ctx, _hp(out), 8), "is_get_eval_counters")
        return dict(unary_full=int(out[0]), unary_gs=int(out[1]), p1_full=int(out[2]), p1_gs=int(out[3]),
                    p1_window_miss=int(out[4]), unary_window_miss=int(out[5]),
                    lutf_spins=int(out[6]), lutf_unit_cycles=int(out[7]),
                    # per phase-1 launch (tile): [full, window misses, ground / sky-only]
                    p1_per_tile=[[int(out[8 + 3 * t + j]) for j in range(3)] for t in range(64)])

    def lut_fused_repaired(self):
        """1 when the last unary call ran its repair launches (test hook, see instance_stixels_core.h)."""
        out = ctypes.c_int(-1)
        _check(lib().is_debug_lut_fused_state(self._ctx, ctypes.byref(out)), "is_debug_lut_fused_state")
        return int(out.value)

    def unary_path(self):
        """(path, repaired): path = 1 when the last unary call computed only the rows the back-trace visits
        (k_unary_path), 0 for the tile path, -1 before any unary call; repaired = calls of this context whose
        path walk was distrusted and redone on the tile path (test hook, see instance_stixels_core.h)."""
        path, rep = ctypes.c_int(-1), ctypes.c_int(-1)
        _check(lib().is_debug_unary_path(self._ctx, ctypes.byref(path), ctypes.byref(rep)), "is_debug_unary_path")
        return int(path.value), int(rep.value)

    def lut_fused_repairs(self):
        """Calls of this context whose fused LUT hand-over was distrusted and repaired (sticky count)."""
        out = ctypes.c_int(-1)
        _check(lib().is_lut_fused_repairs(self._ctx, ctypes.byref(out)), "is_lut_fused_repairs")
        return int(out.value)

    def read_object_lut(self, column):
        """lutT[v][fn] of one stixel column as the last compute call left it (test hook, A4)."""
        out = np.zeros((self.params.rows + 1, self.params.max_dis), np.float32)
        _check(lib().is_debug_read_object_lut(self._ctx, int(column), _hp(out)), "is_debug_read_object_lut")
        return out

    def read_lut_carries(self, column):
        """lutC[k][fn] = lutT[32 k][fn], the object table's block carries of one stixel column as the last walk call
        left them (test hook)."""
        out = np.zeros(((self.params.rows + 31) // 32, self.params.max_dis), np.float32)
        _check(lib().is_debug_read_lut_carries(self._ctx, int(column), _hp(out)), "is_debug_read_lut_carries")
        return out

    def lut_carry_lds(self):
        """(on, pass_columns): on = 1 when the last call's prepare step built the carry rows from a cost table in LDS
        (k_lut_carry), 0 when not, -1 before any call; pass_columns = columns per pass of that kernel's grid."""
        on, n = ctypes.c_int(-1), ctypes.c_int(0)
        _check(lib().is_debug_lut_carry_lds(self._ctx, ctypes.byref(on), ctypes.byref(n)), "is_debug_lut_carry_lds")
        return int(on.value), int(n.value)

    def read_block_summaries(self, column):
        """[n_blocks][24] bound-block summaries of one column after a pairwise call (test hook)."""
        out = np.zeros(4096 * 24, np.float32)
        n = ctypes.c_int(0)
        _check(lib().is_debug_read_block_summaries(self._ctx, int(column), _hp(out), out.size, ctypes.byref(n)),
               "is_debug_read_block_summaries")
        return out[: n.value * 24].reshape(n.value, 24).copy()

    def kernel_times_ms(self):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(lib().is_get_kernel_times_ms(self._ctx, ctypes.byref(a), ctypes.byref(b),
                                            ctypes.byref(c)), "is_get_kernel_times_ms")
        return dict(prepare_ms=a.value, dp_ms=b.value, backtrace_ms=c.value)

    # ---- raw-pointer API (device pointers as ints) -------------------------------------
    def join_columns_ptr(self, d_big, full_cols, median_join, d_joined, n_images, stream=0):
        _check(lib().is_join_columns(self._ctx, d_big, int(full_cols), int(bool(median_join)),
                                     d_joined, int(n_images), stream), "is_join_columns")

    def compute_ptr(self, d_joined, d_seg, ground_function, normalization_ground,
                    inv_sigma2_ground, vhor, pairwise, n_images, d_sections, instances=None,
                    d_cost_table=None, d_index_table=None, stream=0):
        H = self.params.rows
        gf = np.ascontiguousarray(ground_function, np.float32).reshape(n_images, H)
        ng = np.ascontiguousarray(normalization_ground, np.float32).reshape(n_images, H)
        ig = np.ascontiguousarray(inv_sigma2_ground, np.float32).reshape(n_images, H)
        vh = np.ascontiguousarray(vhor, np.int32).reshape(n_images)
        inst = None
        if instances is not None:
            arr = (InstanceBuffers * n_images)(*instances)
            inst = ctypes.cast(arr, ctypes.c_void_p)
        _check(lib().is_compute(self._ctx, d_joined, d_seg, _hp(gf), _hp(ng), _hp(ig), _hp(vh),
                                int(bool(pairwise)), int(n_images), d_sections, inst,
                                d_cost_table, d_index_table, stream), "is_compute")

    def set_ground_model(self, ground_params: GroundParams, log_lut):
        """is_ctx_set_ground_model: the constants and the FastLog table of the device ground model (once per
        context, before compute_road_ptr)."""
        lut = np.ascontiguousarray(log_lut, np.float32)
        gp = GroundParams.from_buffer_copy(ground_params)
        _check(lib().is_ctx_set_ground_model(self._ctx, ctypes.byref(gp), _hp(lut), int(lut.size)),
               "is_ctx_set_ground_model")

    def compute_road_ptr(self, d_joined, d_seg, d_road, pairwise, n_images, d_sections, instances=None,
                         d_cost_table=None, d_index_table=None, vhor_min_hint=-1, stream=0):
        """is_compute_road on raw device pointers: compute_ptr with the ground model built on the device from
        d_road [n_images] RoadParams."""
        inst = None
        if instances is not None:
            arr = (InstanceBuffers * n_images)(*instances)
            inst = ctypes.cast(arr, ctypes.c_void_p)
        _check(lib().is_compute_road(self._ctx, d_joined, d_seg, d_road, int(bool(pairwise)), int(n_images),
                                     d_sections, inst, d_cost_table, d_index_table, int(vhor_min_hint), stream),
               "is_compute_road")

    def read_ground(self, frame):
        """(ground [3][rows] = function | normalization | inv_sigma2, vhor) of one frame as the DP kernels of the
        last compute call read them (test hook)."""
        out = np.zeros((3, self.params.rows), np.float32)
        vh = ctypes.c_int(0)
        _check(lib().is_debug_read_ground(self._ctx, int(frame), _hp(out), ctypes.byref(vh)), "is_debug_read_ground")
        return out, int(vh.value)

    def compute_sweep_ptr(self, d_joined, d_seg, ground_function, normalization_ground, inv_sigma2_ground, vhor,
                          pairwise, n_images, sets, d_sections, instances=None, stream=0):
        """is_compute_sweep on raw device pointers: sets a sequence of SweepSet, instances [n_sets][n_images]
        InstanceBuffers (flat) or None.  Returns the return code and raises nothing (the tests check IS_EINVAL)."""
        H = self.params.rows
        gf = np.ascontiguousarray(ground_function, np.float32).reshape(n_images, H)
        ng = np.ascontiguousarray(normalization_ground, np.float32).reshape(n_images, H)
        ig = np.ascontiguousarray(inv_sigma2_ground, np.float32).reshape(n_images, H)
        vh = np.ascontiguousarray(vhor, np.int32).reshape(n_images)
        arr_sets = (SweepSet * max(len(sets), 1))(*sets)
        inst = None
        if instances is not None:
            arr = (InstanceBuffers * len(instances))(*instances)
            inst = ctypes.cast(arr, ctypes.c_void_p)
        return lib().is_compute_sweep(self._ctx, d_joined, d_seg, _hp(gf), _hp(ng), _hp(ig), _hp(vh),
                                      int(bool(pairwise)), int(n_images), ctypes.cast(arr_sets, ctypes.c_void_p),
                                      len(sets), d_sections, inst, stream)

    def recluster_ptr(self, d_sections, n_images, eps, min_pts, size_filter, instances, stream=0):
        """is_recluster on raw device pointers; returns the return code."""
        arr = (InstanceBuffers * len(instances))(*instances)
        return lib().is_recluster(self._ctx, d_sections, int(n_images), float(eps), int(min_pts), int(size_filter),
                                  ctypes.cast(arr, ctypes.c_void_p), stream)

    def run_sweep(self, sets, joined=None, disparity_big=None, segmentation=None, ground_function=None,
                  normalization_ground=None, inv_sigma2_ground=None, vhor=None, pairwise=False, median_join=False,
                  want_instances=True, canary=0):
        """Runs is_compute_sweep given numpy inputs like run(); every output has a leading [n_sets] axis.  canary > 0:
        the Section and label arrays are allocated with that many guard elements in front and behind, filled with a
        pattern, returned as sections_guard / labels_guard (front, back) for the caller to check."""
        import torch
        p = self.params
        C, H, S = p.cols, p.rows, p.max_sections
        K = len(sets)
        dev = torch.device("cuda", self.device)
        seg = torch.from_numpy(np.ascontiguousarray(segmentation, np.int32)).to(dev)
        n = seg.shape[0]
        stream = torch.cuda.current_stream(dev).cuda_stream
        if joined is None:
            big = torch.from_numpy(np.ascontiguousarray(disparity_big, np.float32)).to(dev)
            d_joined = torch.empty((n, C, H), dtype=torch.float32, device=dev)
            self.join_columns_ptr(big.data_ptr(), big.shape[2], median_join, d_joined.data_ptr(), n, stream)
        else:
            d_joined = torch.from_numpy(np.ascontiguousarray(joined, np.float32)).to(dev)
        g = int(canary)
        pat = 0x5A5A5A5A
        sec_all = torch.full((K * n * C * S * 8 + 2 * g * 8,), pat, dtype=torch.int32, device=dev)
        sections = sec_all[g * 8: g * 8 + K * n * C * S * 8]
        inst_t, inst_s, lab_all = None, None, None
        if want_instances:
            com = torch.zeros((K, n, INSTANCE_CLASSES, C * S, 2), dtype=torch.float32, device=dev)
            idx = torch.zeros((K, n, INSTANCE_CLASSES, C * S, 2), dtype=torch.int32, device=dev)
            core = torch.zeros((K, n, INSTANCE_CLASSES, C * S), dtype=torch.uint8, device=dev)
            per = torch.zeros((K, n, INSTANCE_CLASSES), dtype=torch.int32, device=dev)
            lab_all = torch.full((K * n * INSTANCE_CLASSES * C * S + 2 * g,), -9, dtype=torch.int32, device=dev)
            lab = lab_all[g: g + K * n * INSTANCE_CLASSES * C * S].view(K, n, INSTANCE_CLASSES, C * S)
            inst_t = (com, idx, core, per, lab)
            inst_s = [InstanceBuffers(com[k, i].data_ptr(), idx[k, i].data_ptr(), core[k, i].data_ptr(),
                                      per[k, i].data_ptr(), lab[k, i].data_ptr(), None)
                      for k in range(K) for i in range(n)]
        rc = self.compute_sweep_ptr(d_joined.data_ptr(), seg.data_ptr(), ground_function, normalization_ground,
                                    inv_sigma2_ground, vhor, pairwise, n, sets, sections.data_ptr(), inst_s, stream)
        _check(rc, "is_compute_sweep")
        torch.cuda.synchronize(dev)
        out = dict(joined=d_joined.cpu().numpy(),
                   sections=sections.cpu().numpy().view(SECTION_DTYPE).reshape(K, n, C, S))
        if g:
            a = sec_all.cpu().numpy()
            out["sections_guard"] = (a[:g * 8].copy(), a[a.size - g * 8:].copy(), np.int32(pat))
        if want_instances:
            out["inst_centerofmass"] = inst_t[0].cpu().numpy()
            out["inst_indices"] = inst_t[1].cpu().numpy()
            out["inst_core"] = inst_t[2].cpu().numpy()
            out["inst_per_class"] = inst_t[3].cpu().numpy()
            out["inst_labels"] = inst_t[4].cpu().numpy()
            if g:
                a = lab_all.cpu().numpy()
                out["labels_guard"] = (a[:g].copy(), a[a.size - g:].copy(), np.int32(-9))
        return out

    # ---- torch-tensor convenience API ----------------------------------------------------
    def run(self, disparity_big=None, joined=None, segmentation=None, ground_function=None,
            normalization_ground=None, inv_sigma2_ground=None, vhor=None, pairwise=False,
            median_join=False, want_tables=False, want_instances=True, road=None, vhor_min_hint=-1):
        """Runs a batch given numpy inputs; returns numpy outputs (one sync at the end).

        disparity_big [n][H][W] or joined [n][C][H]; segmentation [n][C][CH][P2S].  road (n records of ROAD_DTYPE):
        is_compute_road with the records uploaded, in place of is_compute with the four host arrays."""
        import torch
        p = self.params
        C, H, S = p.cols, p.rows, p.max_sections
        dev = torch.device("cuda", self.device)
        seg = torch.from_numpy(np.ascontiguousarray(segmentation, np.int32)).to(dev)
        n = seg.shape[0]
        stream = torch.cuda.current_stream(dev).cuda_stream
        if joined is None:
            big = torch.from_numpy(np.ascontiguousarray(disparity_big, np.float32)).to(dev)
            assert big.shape[0] == n and big.shape[1] == H
            d_joined = torch.empty((n, C, H), dtype=torch.float32, device=dev)
            self.join_columns_ptr(big.data_ptr(), big.shape[2], median_join, d_joined.data_ptr(), n,
                                  stream)
        else:
            d_joined = torch.from_numpy(np.ascontiguousarray(joined, np.float32)).to(dev)
        sections = torch.empty((n, C, S, 8), dtype=torch.int32, device=dev)
        cost = torch.empty((n, C, H, 3), dtype=torch.float32, device=dev) if want_tables else None
        index = torch.empty((n, C, H, 3), dtype=torch.int32, device=dev) if want_tables else None
        inst_t, inst_s = None, None
        if want_instances:
            com = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.float32, device=dev)
            idx = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.int32, device=dev)
            core = torch.zeros((n, INSTANCE_CLASSES, C * S), dtype=torch.uint8, device=dev)
            per = torch.zeros((n, INSTANCE_CLASSES), dtype=torch.int32, device=dev)
            lab = torch.full((n, INSTANCE_CLASSES, C * S), -9, dtype=torch.int32, device=dev)
            inst_t = (com, idx, core, per, lab)
            inst_s = [InstanceBuffers(com[i].data_ptr(), idx[i].data_ptr(), core[i].data_ptr(),
                                      per[i].data_ptr(), lab[i].data_ptr(), None)
                      for i in range(n)]
        if road is not None:
            rp = np.ascontiguousarray(road, ROAD_DTYPE).reshape(n)
            d_road = torch.from_numpy(rp.view(np.int32).reshape(n, 4)).to(dev)
            self.compute_road_ptr(d_joined.data_ptr(), seg.data_ptr(), d_road.data_ptr(), pairwise, n,
                                  sections.data_ptr(), inst_s, cost.data_ptr() if cost is not None else None,
                                  index.data_ptr() if index is not None else None, vhor_min_hint, stream)
        else:
            self.compute_ptr(d_joined.data_ptr(), seg.data_ptr(), ground_function,
                             normalization_ground, inv_sigma2_ground, vhor, pairwise, n,
                             sections.data_ptr(), inst_s,
                             cost.data_ptr() if cost is not None else None,
                             index.data_ptr() if index is not None else None, stream)
        torch.cuda.synchronize(dev)
        out = dict(joined=d_joined.cpu().numpy(),
                   sections=sections.cpu().numpy().view(SECTION_DTYPE).reshape(n, C, S))
        if want_tables:
            out["cost_table"] = cost.cpu().numpy()
            out["index_table"] = index.cpu().numpy()
        if want_instances:
            out["inst_centerofmass"] = inst_t[0].cpu().numpy()
            out["inst_indices"] = inst_t[1].cpu().numpy()
            out["inst_core"] = inst_t[2].cpu().numpy()
            out["inst_per_class"] = inst_t[3].cpu().numpy()
            out["inst_labels"] = inst_t[4].cpu().numpy()
        return out

    def cluster_instances(self, centerofmass, core_candidates, per_class):
        """Size-filtered DBSCAN (is_cluster_instances) of one image's candidate arrays given as
        numpy: centerofmass [8][n_slots][2] f32, core_candidates [8][n_slots] u8, per_class [8].
        Returns (labels [8][n_slots] int32, packed triples [total][3])."""
        import torch
        p = self.params
        slots = p.cols * p.max_sections
        dev = torch.device("cuda", self.device)
        com = torch.from_numpy(np.ascontiguousarray(centerofmass, np.float32)).to(dev)
        cand = torch.from_numpy(np.ascontiguousarray(core_candidates, np.uint8)).to(dev)
        per = torch.from_numpy(np.ascontiguousarray(per_class, np.int32)).to(dev)
        assert com.shape == (INSTANCE_CLASSES, slots, 2) and cand.shape == (INSTANCE_CLASSES, slots)
        idx = torch.zeros((INSTANCE_CLASSES, slots, 2), dtype=torch.int32, device=dev)
        idx[:, :, 0] = torch.arange(INSTANCE_CLASSES, device=dev, dtype=torch.int32)[:, None]
        idx[:, :, 1] = torch.arange(slots, device=dev, dtype=torch.int32)[None, :]
        lab = torch.full((INSTANCE_CLASSES, slots), -9, dtype=torch.int32, device=dev)
        packed = torch.full((1 + 3 * INSTANCE_CLASSES * slots,), -9, dtype=torch.int32, device=dev)
        ib = InstanceBuffers(com.data_ptr(), idx.data_ptr(), cand.data_ptr(), per.data_ptr(),
                             lab.data_ptr(), packed.data_ptr())
        _check(lib().is_cluster_instances(self._ctx, ctypes.byref(ib),
                                          torch.cuda.current_stream(dev).cuda_stream),
               "is_cluster_instances")
        torch.cuda.synchronize(dev)
        pk = packed.cpu().numpy()
        return lab.cpu().numpy(), pk[1:1 + 3 * int(pk[0])].reshape(-1, 3)


def comm_unique_id():
    """128 bytes of an ncclUniqueId (is_comm_unique_id): created by one rank, handed to all."""
    buf = ctypes.create_string_buffer(128)
    _check(lib().is_comm_unique_id(buf, 128), "is_comm_unique_id")
    return buf.raw


def comm_init_rank(nranks, uid, rank):
    """An RCCL communicator on the current device (is_comm_init_rank) -> ncclComm_t as int."""
    comm = ctypes.c_void_p()
    _check(lib().is_comm_init_rank(ctypes.byref(comm), int(nranks), ctypes.c_char_p(uid), int(rank)),
           "is_comm_init_rank")
    return comm.value


def comm_destroy(comm):
    _check(lib().is_comm_destroy(ctypes.c_void_p(comm)), "is_comm_destroy")


def gather_sections_ptr(comm, dst, columns, d_counts, d_offsets, d_packed, d_all_counts, d_all_packed,
                        cap_sections, stream=0):
    """is_gather_sections on raw device pointers; returns the per-rank section totals (dst: all of them)."""
    cols = np.ascontiguousarray(columns, np.int32)
    totals = np.zeros(cols.size, np.int64)
    _check(lib().is_gather_sections(ctypes.c_void_p(comm), int(dst), _hp(cols), d_counts, d_offsets, d_packed,
                                    d_all_counts, d_all_packed, int(cap_sections), _hp(totals), stream),
           "is_gather_sections")
    return totals


def pack_sections_ptr(d_sections, n_columns, max_sections, d_counts, d_offsets, d_packed, stream=0):
    """is_pack_sections on raw device pointers (ints)."""
    _check(lib().is_pack_sections(d_sections, int(n_columns), int(max_sections), d_counts, d_offsets,
                                  d_packed, stream), "is_pack_sections")


def unpack_sections_ptr(d_counts, d_offsets, d_packed, n_columns, max_sections, d_sections, stream=0):
    _check(lib().is_unpack_sections(d_counts, d_offsets, d_packed, int(n_columns), int(max_sections),
                                    d_sections, stream), "is_unpack_sections")


def render_sections_ptr(stream=0, class_to_label=None, **fields):
    """is_render_sections on raw device pointers (ints): fields are those of RenderArgs (d_sections, n_images,
    realcols, max_sections, rows, cols, d_label, ...); class_to_label: a host sequence of label values, None for
    Cityscapes trainId -> labelId.  Asynchronous on `stream`."""
    a = RenderArgs(**fields)
    table = None
    if class_to_label is not None:
        table = np.ascontiguousarray(class_to_label, np.uint8)
        a.h_class_to_label, a.n_classes = table.ctypes.data, table.size
    _check(lib().is_render_sections(ctypes.byref(a), ctypes.c_void_p(int(stream))), "is_render_sections")


def instance_overlap_ptr(stream=0, **fields):
    """is_instance_overlap on raw device pointers (ints): fields are those of InstanceOverlapArgs.  Asynchronous
    on `stream`."""
    a = InstanceOverlapArgs(**fields)
    _check(lib().is_instance_overlap(ctypes.byref(a), ctypes.c_void_p(int(stream))), "is_instance_overlap")


def stixel_world_ptr(alpha_ground, vhor, stream=0, **fields):
    """is_stixel_world on raw device pointers (ints): fields are those of WorldArgs; alpha_ground / vhor: the road
    of every frame (host sequences, library-convention vhor).  Asynchronous on `stream`."""
    a = WorldArgs(**fields)
    alpha = np.ascontiguousarray(alpha_ground, np.float32)
    vh = np.ascontiguousarray(vhor, np.int32)
    a.h_alpha_ground, a.h_vhor = alpha.ctypes.data, vh.ctypes.data
    _check(lib().is_stixel_world(ctypes.byref(a), ctypes.c_void_p(int(stream))), "is_stixel_world")


def assign_instances_gt_ptr(stream=0, label_ids=None, **fields):
    """is_assign_instances_gt on raw device pointers (ints): fields are those of AssignGtArgs (d_sections,
    d_gt_instance, n_images, rows, cols, realcols, max_sections, min_fraction, gt_is_train_ids, d_section_instance,
    d_section_votes); label_ids: a host sequence of the eight labelIds of classes 11..18, None for Cityscapes.
    Asynchronous on `stream`."""
    a = AssignGtArgs(**fields)
    ids = None
    if label_ids is not None:
        ids = np.ascontiguousarray(label_ids, np.int32)
        if ids.size != 8:
            raise ValueError("label_ids must hold 8 ids")
        a.h_label_ids = ids.ctypes.data
    _check(lib().is_assign_instances_gt(ctypes.byref(a), ctypes.c_void_p(int(stream))), "is_assign_instances_gt")


def pack_section_labels_ptr(d_section_instance, n_images, realcols, max_sections, capacity, d_packed, stream=0):
    """is_pack_section_labels on raw device pointers (ints)."""
    _check(lib().is_pack_section_labels(d_section_instance, int(n_images), int(realcols), int(max_sections),
                                        int(capacity), d_packed, ctypes.c_void_p(int(stream))),
           "is_pack_section_labels")


def instance_disparity_scratch_bytes(n_images, realcols, max_sections, capacity):
    """is_instance_disparity_scratch_bytes: the scratch a call of that shape needs (0: a shape the call refuses)."""
    return int(lib().is_instance_disparity_scratch_bytes(int(n_images), int(realcols), int(max_sections),
                                                         int(capacity)))


def cluster_instance_disparity_ptr(instances, stream=0, **fields):
    """is_cluster_instance_disparity on raw device pointers (ints): fields are those of InstanceDisparityArgs except
    `instances`, a sequence of n_images InstanceBuffers.  Asynchronous on `stream`; returns the return code and raises
    nothing (the tests check IS_EINVAL)."""
    a = InstanceDisparityArgs(**fields)
    arr = (InstanceBuffers * max(len(instances), 1))(*instances)
    a.instances = ctypes.cast(arr, ctypes.c_void_p)
    return lib().is_cluster_instance_disparity(ctypes.byref(a), ctypes.c_void_p(int(stream)))


def instance_objects_ptr(stream=0, **fields):
    """is_instance_objects on raw device pointers (ints): fields are those of InstanceObjectsArgs.  Asynchronous on
    `stream`."""
    a = InstanceObjectsArgs(**fields)
    _check(lib().is_instance_objects(ctypes.byref(a), ctypes.c_void_p(int(stream))), "is_instance_objects")


def road_choose_batch_ptr(road_ctx, n_images, d_lines, d_total, d_overflow, max_lines, cy, baseline, focal,
                          min_pitch, max_pitch, fallback, d_road, d_status, stream=0):
    """is_road_choose_batch on raw device pointers; fallback = (vhor_image, tilt, height, alpha).  Returns the return
    code (the tests check IS_EINVAL)."""
    fb = RoadParams(int(fallback[0]), float(fallback[1]), float(fallback[2]), float(fallback[3]))
    return lib().is_road_choose_batch(road_ctx, int(n_images), d_lines, d_total, d_overflow, int(max_lines), cy,
                                      baseline, focal, min_pitch, max_pitch, fb, d_road, d_status, stream)


def _with_reserved(cls, fields):
    reserved = fields.pop("reserved", None)
    a = cls(**fields)
    if reserved is not None:
        for i, v in enumerate(reserved):
            a.reserved[i] = int(v)
    return a


def _args_ptr(entry, **defaults):
    """The function `entry`_ptr (without "is_") of an entry point of _ARGS_ENTRY that takes nothing but the struct:
    (stream=0, **fields) -> the return code.  defaults: field values other than the zeros of ctypes."""
    cls = _ARGS_ENTRY[entry]
    fill = _with_reserved if hasattr(cls, "reserved") else lambda cls, fields: cls(**fields)

    def ptr(stream=0, **fields):
        a = fill(cls, {**defaults, **fields})
        return getattr(lib(), entry)(ctypes.byref(a), ctypes.c_void_p(int(stream)))
    ptr.__name__ = ptr.__qualname__ = entry[3:] + "_ptr"
    ptr.__doc__ = (f"{entry} on raw device pointers (ints): fields are those of {cls.__name__}" +
                   "".join(f" ({k} defaults to {v} here)" for k, v in defaults.items()) +
                   ".  Asynchronous on `stream`; returns the return code and raises nothing (the tests check IS_EINVAL).")
    return ptr


gt_instance_targets_ptr = _args_ptr("is_gt_instance_targets")
offset_loss_ptr = _args_ptr("is_offset_loss")
segmentation_head_ptr = _args_ptr("is_segmentation_head", clamp_channel=-1)
segmentation_head_backward_ptr = _args_ptr("is_segmentation_head_backward")
semantic_nll_ptr = _args_ptr("is_semantic_nll")
semantic_nll_up_ptr = _args_ptr("is_semantic_nll_up")
conv3x3_bn_relu_ptr = _args_ptr("is_conv3x3_bn_relu")
conv_bn_ptr = _args_ptr("is_conv_bn")
conv_bn_stride_ptr = _args_ptr("is_conv_bn_stride")
stem_ptr = _args_ptr("is_stem")
conv_bn_backward_ptr = _args_ptr("is_conv_bn_backward")
conv_bn_stride_backward_ptr = _args_ptr("is_conv_bn_stride_backward")
stem_backward_ptr = _args_ptr("is_stem_backward")


@functools.lru_cache(maxsize=None)
def _guard_patterns():
    """{torch dtype: (the allocation's dtype, the fill value, the pattern as _Fresh.guards() gives it)}; made on first
    use, as torch is imported late."""
    import torch
    half = (torch.int16, 0x5A5A, np.uint16(0x5A5A))
    return {torch.float32: (torch.float32, -12345.0, np.float32(-12345.0)), torch.float16: half, torch.bfloat16: half,
            torch.int32: (torch.int32, 0x5A5A5A5A, np.int32(0x5A5A5A5A)),
            torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A, np.int64(0x5A5A5A5A5A5A5A5A)),
            torch.uint8: (torch.uint8, 0xA5, np.uint8(0xA5))}


class _Fresh:
    """The tensors one call of an entry point allocates on `dev`.  canary = 0: plain torch.empty, nothing is recorded.
    canary > 0: every tensor is the middle of one torch.full allocation with that many guard elements of the dtype's
    pattern in front and behind, and guards() reads them back.  A half's pattern is given as its 16 bits, 0x5A5A, a
    finite value in both half formats, so its allocation is int16 and the tensor reinterprets it."""
    def __init__(self, dev, canary):
        self.dev, self.g, self._named = dev, int(canary), {}

    def new(self, name, shape, dtype, g=None):
        """A tensor of `shape`, recorded as `name`; g: a guard length other than the canary."""
        import torch
        g = self.g if g is None else g
        if not g:
            return torch.empty(shape, dtype=dtype, device=self.dev)
        whole, fill, pattern = _guard_patterns()[dtype]
        numel = math.prod(shape)
        full = torch.full((numel + 2 * g,), fill, dtype=whole, device=self.dev)
        self._named[name] = (full, g, pattern)
        flat = full[g: g + numel]
        return (flat if whole is dtype else flat.view(dtype)).view(shape)

    def rows(self, rows):
        """new() for the wanted ones of the rows (name, want, shape, dtype): ({name: tensor}, {name: data pointer,
        None where not wanted})."""
        out, ptr = {}, {}
        for name, want, shape, dtype in rows:
            ptr[name] = None
            if want:
                out[name] = self.new(name, shape, dtype)
                ptr[name] = out[name].data_ptr()
        return out, ptr

    def scratch(self, nbytes):
        """The uint8 scratch of a call, recorded as "scratch".  Its guard is whole 16 bytes, which keeps it 16-byte
        aligned (torch's allocations are)."""
        import torch
        return self.new("scratch", (nbytes,), torch.uint8, (self.g + 15) // 16 * 16)

    def guards(self):
        """{name: (front, back, pattern)} as numpy copies of the guard elements (one synchronisation)."""
        import torch
        out = {}
        for name, (full, g, pattern) in self._named.items():
            h = full.view(torch.uint8).cpu().numpy().view(pattern.dtype)
            out[name] = (h[:g].copy(), h[h.size - g:].copy(), pattern)
        return out


def flip_and_pad(cnn_out, rows_power2_segmentation, device=0):
    """CNN output [n][CH][Hs][Ws] float32 (numpy) -> DP input [n][Ws][CH][P2S] int32 (numpy)."""
    import torch
    dev = torch.device("cuda", device)
    x = torch.from_numpy(np.ascontiguousarray(cnn_out, np.float32)).to(dev)
    n, CH, Hs, Ws = x.shape
    out = torch.empty((n, Ws, CH, int(rows_power2_segmentation)), dtype=torch.int32, device=dev)
    _check(lib().is_flip_and_pad(x.data_ptr(), out.data_ptr(), n, CH, Hs, Ws,
                                 int(rows_power2_segmentation),
                                 torch.cuda.current_stream(dev).cuda_stream), "is_flip_and_pad")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def mode_downsample_ptr(d_src, dtype, n_images, rows, cols, d_dst, stream=0):
    """is_mode_downsample on raw device pointers (ints).  Returns the return code and raises nothing (the tests check
    IS_EINVAL)."""
    return lib().is_mode_downsample(d_src, int(dtype), int(n_images), int(rows), int(cols), d_dst,
                                    ctypes.c_void_p(int(stream)))


def gt_targets_scratch_bytes(n_images, rows, cols, with_disparity=False, capacity=0):
    """is_gt_targets_scratch_bytes: the scratch a call of that shape needs (0: a shape the call refuses)."""
    return int(lib().is_gt_targets_scratch_bytes(int(n_images), int(rows), int(cols), int(bool(with_disparity)),
                                                 int(capacity)))


def _torch_dtype_code(t):
    import torch
    codes = {torch.uint8: DTYPE_UINT8, torch.uint16: DTYPE_UINT16, torch.int32: DTYPE_INT32}
    if t.dtype not in codes:
        raise CoreError(f"dtype {t.dtype} is none of uint8, uint16, int32")
    return codes[t.dtype]


def _head_codes(halves_only=False):
    """{torch dtype: IS_HEAD_* code} of the feature dtypes: float32, float16 and bfloat16, or the two halves alone."""
    import torch
    codes = {torch.float32: HEAD_F32, torch.float16: HEAD_F16, torch.bfloat16: HEAD_BF16}
    if halves_only:
        del codes[torch.float32]
    return codes


def _f32_on(v, dev):
    """v, a tensor or an array, as a contiguous float32 tensor on `dev`."""
    import torch
    t = v if torch.is_tensor(v) else torch.tensor(np.asarray(v, np.float32))
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _current_stream(dev):
    """The current torch stream of device `dev`, as the C ABI takes it."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _scratch_or_raise(fn, shape, **unnamed):
    """The scratch bytes fn(**shape, **unnamed) of a call; CoreError with the shape where the C ABI refuses it (0)."""
    nbytes = fn(**shape, **unnamed)
    if nbytes == 0:
        what = "the shape or the capacity" if "capacity" in shape else "the shape"
        raise CoreError(f"is_{fn.__name__} refuses {what} ({', '.join(f'{k} {v}' for k, v in shape.items())})")
    return nbytes


def _planes_in_place(t, planes):
    """t [n][C >= planes][H][W] can be read or written where it is: each frame's planes are contiguous, the batch
    stride is free."""
    n, _, H, W = t.shape
    return t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W and (n == 1 or t.stride(0) >= planes * H * W)


def _frame_planes(t, planes):
    """(tensor, image stride in elements): t itself where _planes_in_place, else a contiguous copy."""
    if not _planes_in_place(t, planes):
        t = t.contiguous()
    return t, t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2] * t.shape[3]


def _until_keys_fit(call, count, cells, capacity, read_back):
    """call(capacity), repeated with the frames' largest key count (read back from `count`: one synchronisation) while
    that is above the capacity the call worked with; capacity 0 is the C ABI's default, min(256, cells)."""
    while True:
        call(capacity)
        if not read_back:
            return
        most = int(count.max().item())
        if most <= (int(capacity) if capacity else min(256, cells)):
            return
        capacity = most   # (never above the cells of a frame; above IS_GT_TARGETS_MAX_CAPACITY it is refused)


def mode_downsample(t):
    """The reference's ModeDownsample(8) of a device tensor [n][rows][cols] (or [rows][cols]) of dtype uint8, uint16
    or int32: the most frequent value of every 8x8 block, the smallest among equals.  A tensor of the same dtype
    [n][rows / 8][cols / 8] on the input's device, enqueued on the current torch stream."""
    import torch
    if not t.is_cuda:
        raise CoreError("mode_downsample takes a device tensor")
    x = t.contiguous()
    if x.dim() not in (2, 3):
        raise CoreError("mode_downsample takes [n][rows][cols] or [rows][cols]")
    n = x.shape[0] if x.dim() == 3 else 1
    rows, cols = x.shape[-2:]
    with torch.cuda.device(x.device):
        out = torch.empty(tuple(x.shape[:-2]) + (rows // 8, cols // 8), dtype=x.dtype, device=x.device)
        _check(lib().is_mode_downsample(x.data_ptr(), _torch_dtype_code(x), n, rows, cols, out.data_ptr(),
                                        torch.cuda.current_stream(x.device).cuda_stream), "is_mode_downsample")
    return out


def gt_instance_targets(gt_instance, disparity_u16=None, segmentation=None, rows_power2_segmentation=None,
                        out=None, capacity=0, return_key_count=False):
    """The ground-truth offset targets of a batch (is_gt_instance_targets, instance_stixels_core.h f11).

    gt_instance      device int32 [n][rows][cols], rows and cols multiples of 8
    disparity_u16    optional device uint16 [n][rows][cols]: the targets get the disparity plane in front
    segmentation     optional device int32 [n][cols / 8][21][P2S]: channels 19 and 20 are rewritten in place
    rows_power2_segmentation   its last dimension (default: taken from the tensor)
    out              optional device float32 [n][2 or 3][rows / 8][cols / 8] to write the targets into

    Returns (targets, ids8) as torch tensors on the inputs' device, enqueued on the current torch stream; with
    return_key_count the frames' key counts as a third tensor.  With a disparity image the frames' key counts are
    read back (one synchronisation), and a frame with more keys than `capacity` (0: the default of the C ABI) makes
    the call repeat with that count, so the result is always complete."""
    import torch
    g = gt_instance
    if not g.is_cuda or g.dtype != torch.int32 or g.dim() != 3:
        raise CoreError("gt_instance must be a device int32 tensor [n][rows][cols]")
    g = g.contiguous()
    dev = g.device
    n, rows, cols = g.shape
    planes = 3 if disparity_u16 is not None else 2
    d = None
    if disparity_u16 is not None:
        d = disparity_u16
        if d.device != dev or d.dtype != torch.uint16 or tuple(d.shape) != tuple(g.shape):
            raise CoreError("disparity_u16 must be a uint16 tensor of gt_instance's shape and device")
        d = d.contiguous()
    Hs, Ws = rows // 8, cols // 8
    if out is None:
        out = torch.empty((n, planes, Hs, Ws), dtype=torch.float32, device=dev)
    elif (out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (n, planes, Hs, Ws)
          or not out.is_contiguous()):
        raise CoreError(f"out must be a contiguous float32 tensor {(n, planes, Hs, Ws)} on gt_instance's device")
    p2s = 0
    if segmentation is not None:
        s = segmentation
        p2s = int(rows_power2_segmentation) if rows_power2_segmentation is not None else int(s.shape[-1])
        if (s.device != dev or s.dtype != torch.int32 or tuple(s.shape) != (n, Ws, 21, p2s)
                or not s.is_contiguous()):
            raise CoreError(f"segmentation must be a contiguous int32 tensor {(n, Ws, 21, p2s)} on gt_instance's device")
    with torch.cuda.device(dev):
        ids8 = torch.empty((n, Hs, Ws), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)

        def call(capacity):
            shape = dict(n_images=n, rows=rows, cols=cols, capacity=capacity)
            nbytes = _scratch_or_raise(gt_targets_scratch_bytes, shape, with_disparity=d is not None)
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            a = GtTargetsArgs(d_gt_instance=g.data_ptr(), d_disparity_u16=d.data_ptr() if d is not None else None,
                              n_images=n, rows=rows, cols=cols, d_targets=out.data_ptr(), target_planes=planes,
                              d_ids8=ids8.data_ptr(),
                              d_segmentation=segmentation.data_ptr() if segmentation is not None else None,
                              rows_power2_segmentation=p2s, channels=21 if segmentation is not None else 0,
                              capacity=int(capacity), d_scratch=scratch.data_ptr(), scratch_bytes=nbytes,
                              d_key_count=count.data_ptr())
            _check(lib().is_gt_instance_targets(ctypes.byref(a), _current_stream(dev)), "is_gt_instance_targets")
        _until_keys_fit(call, count, Hs * Ws, capacity, read_back=d is not None)
    return (out, ids8, count) if return_key_count else (out, ids8)


OFFSET_LOSS_WEIGHTS = (1e-3, 1e-4, 1e-3, 1e-4)   # offset_mean, offset_variance, disparity_mean, disparity_variance


def offset_loss_scratch_bytes(n_images, planes, rows8, cols8, capacity=0):
    """is_offset_loss_scratch_bytes: the scratch a call of that shape needs (0: a shape the call refuses)."""
    return int(lib().is_offset_loss_scratch_bytes(int(n_images), int(planes), int(rows8), int(cols8), int(capacity)))


def offset_loss(prediction, ids8, disparity8_u16=None, weights=OFFSET_LOSS_WEIGHTS, abs_variance=False, capacity=0,
                check=True, return_key_count=False):
    """The reference's OffsetLossSL / DisparityOffsetLossSL of a batch with the gradient (is_offset_loss,
    instance_stixels_core.h f12).

    prediction       device float32 [n][2 or 3][Hs][Ws]; a channel slice of a wider tensor (outputs[:, -3:]) is read
                     in place when its planes are contiguous, anything else is copied
    ids8             device int32 [n][Hs][Ws]: the instance ids mode-downsampled by 8
    disparity8_u16   device uint16 [n][Hs][Ws] with 3 planes: the raw disparity mode-downsampled by 8
    weights          (offset_mean, offset_variance, disparity_mean, disparity_variance), rounded to float32

    Returns (loss5, terms, grad): float32 [5] (loss and the four batch sums), [n][4] and the gradient in the
    prediction's shape, on the inputs' device, enqueued on the current torch stream.  With check=True the key counts
    are read back (one synchronisation) and a frame with more keys than `capacity` (0: the default of the C ABI) makes
    the call repeat with that count; with check=False such a batch returns NaN losses and an unwritten gradient."""
    import torch
    p = prediction
    if not p.is_cuda or p.dtype != torch.float32 or p.dim() != 4 or p.shape[1] not in (2, 3):
        raise CoreError("prediction must be a device float32 tensor [n][2 or 3][Hs][Ws]")
    dev = p.device
    n, planes, Hs, Ws = p.shape
    p, p_stride = _frame_planes(p, planes)
    if ids8.device != dev or ids8.dtype != torch.int32 or tuple(ids8.shape) != (n, Hs, Ws):
        raise CoreError(f"ids8 must be an int32 tensor {(n, Hs, Ws)} on the prediction's device")
    i8 = ids8.contiguous()
    d8 = None
    if planes == 3:
        d8 = disparity8_u16
        if d8 is None or d8.device != dev or d8.dtype != torch.uint16 or tuple(d8.shape) != (n, Hs, Ws):
            raise CoreError(f"3 planes need disparity8_u16, a uint16 tensor {(n, Hs, Ws)} on the prediction's device")
        d8 = d8.contiguous()
    elif disparity8_u16 is not None:
        raise CoreError("disparity8_u16 goes with 3 planes")
    w = [float(v) for v in weights]
    with torch.cuda.device(dev):
        loss5 = torch.empty((5,), dtype=torch.float32, device=dev)
        terms = torch.empty((n, 4), dtype=torch.float32, device=dev)
        grad = torch.empty((n, planes, Hs, Ws), dtype=torch.float32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)

        def call(capacity):
            nbytes = _scratch_or_raise(offset_loss_scratch_bytes,
                                       dict(n_images=n, planes=planes, rows8=Hs, cols8=Ws, capacity=capacity))
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            a = OffsetLossArgs(d_prediction=p.data_ptr(), prediction_image_stride=p_stride, d_ids8=i8.data_ptr(),
                               d_disparity8_u16=d8.data_ptr() if d8 is not None else None, n_images=n, planes=planes,
                               rows8=Hs, cols8=Ws, w_offset_mean=w[0], w_offset_variance=w[1], w_disparity_mean=w[2],
                               w_disparity_variance=w[3], abs_variance=int(bool(abs_variance)),
                               d_loss=loss5.data_ptr(), d_terms=terms.data_ptr(), d_grad=grad.data_ptr(),
                               grad_image_stride=planes * Hs * Ws, capacity=int(capacity),
                               d_scratch=scratch.data_ptr(), scratch_bytes=nbytes, d_key_count=count.data_ptr())
            _check(lib().is_offset_loss(ctypes.byref(a), _current_stream(dev)), "is_offset_loss")
        _until_keys_fit(call, count, Hs * Ws, capacity, read_back=check)
    return (loss5, terms, grad, count) if return_key_count else (loss5, terms, grad)


def segmentation_head(features, weight, bias, n_classes, rows_power2_segmentation, want_cnn_out=False, clamp=None,
                      device=0, want_segmentation=True, canary=0):
    """The CNN's segmentation head of a batch in one launch (is_segmentation_head, instance_stixels_core.h f13): the
    1x1 convolution `seg`, -log_softmax over the first n_classes channels, the regression channels passed through
    (clamp = (channel, lo, hi) clamps one of them) and FlipAndPad, with the numerics the header fixes.

    features    [n][K][rows8][cols8] float32, float16 or bfloat16: a torch tensor on the device, or an array that is
                copied to cuda:`device`; made contiguous NCHW, its dtype selects the kernel's
    weight      [channels][K] (or seg.weight's [channels][K][1][1]) and bias [channels]: tensors or arrays, float32

    Returns the DP input, an int32 tensor [n][cols8][channels][rows_power2_segmentation] on the features' device
    (what Core.compute_ptr, ComputeBatch and SweepBatch take), and with want_cnn_out the float32 network output
    [n][channels][rows8][cols8] behind it; enqueued on the current torch stream.  want_segmentation=False leaves
    the int tensor out (then want_cnn_out is implied and the float tensor alone is returned).  canary > 0: both
    outputs are allocated with that many guard words in front and behind, filled with a pattern, and a dict
    {"segmentation": (front, back, pattern), "cnn_out": ...} of numpy copies of the guards is returned last (one
    synchronisation)."""
    import torch
    x = features
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", device))
    if not x.is_cuda or x.dim() != 4:
        raise CoreError("features must be a device tensor [n][K][rows8][cols8]")
    codes = _head_codes()
    if x.dtype not in codes:
        raise CoreError(f"features dtype {x.dtype} is none of float32, float16, bfloat16")
    x = x.contiguous()
    dev = x.device
    n, K, Hs, Ws = x.shape
    b = _f32_on(bias, dev).reshape(-1)
    CH = int(b.numel())
    w = _f32_on(weight, dev).reshape(CH, -1)
    if w.shape[1] != K:
        raise CoreError(f"weight holds {w.shape[1]} values per channel, the features have K = {K}")
    P2S = int(rows_power2_segmentation)
    if not want_segmentation:
        want_cnn_out = True
    with torch.cuda.device(dev):
        fresh = _Fresh(dev, canary)
        out, ptr = fresh.rows((("segmentation", want_segmentation, (n, Ws, CH, P2S), torch.int32),
                               ("cnn_out", want_cnn_out, (n, CH, Hs, Ws), torch.float32)))
        a = SegmentationHeadArgs(d_features=x.data_ptr(), dtype=codes[x.dtype], n_images=n, K=K, rows8=Hs, cols8=Ws,
                                 d_weight=w.data_ptr(), d_bias=b.data_ptr(), n_classes=int(n_classes),
                                 n_regression=CH - int(n_classes), rows_power2_segmentation=P2S, clamp_channel=-1,
                                 d_cnn_out=ptr["cnn_out"], d_segmentation=ptr["segmentation"])
        if clamp is not None:
            a.clamp_channel, a.clamp_lo, a.clamp_hi = int(clamp[0]), float(clamp[1]), float(clamp[2])
        _check(lib().is_segmentation_head(ctypes.byref(a), _current_stream(dev)), "is_segmentation_head")
        out = list(out.values())
        if fresh.g:
            out.append(fresh.guards())
    return out[0] if len(out) == 1 else tuple(out)


def _conv_pack(prefix, with_kernel, weight, dtype, device):
    """The body of conv3x3_pack_weights and conv_pack_weights: the entry points `prefix`_packed_bytes and
    `prefix`_pack_weights of the C ABI, which take the kernel size k of a weight [..][k][k] (with_kernel: f18) or are
    3x3 alone (f17).  Every refusal is made before the weight goes to a device."""
    import torch
    codes = _head_codes(halves_only=True)
    if dtype not in codes:
        raise CoreError(f"dtype {dtype} is neither torch.float16 nor torch.bfloat16")
    w = weight if torch.is_tensor(weight) else torch.from_numpy(np.ascontiguousarray(weight, np.float32))
    if w.dim() != 4 or (w.shape[2] != w.shape[3] if with_kernel else tuple(w.shape[2:]) != (3, 3)):
        raise CoreError(f"weight must be [channels_out][channels_in]{'[k][k]' if with_kernel else '[3][3]'}")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    k = (int(w.shape[2]),) if with_kernel else ()
    nbytes = int(getattr(lib(), prefix + "_packed_bytes")(cout, cin, *k, codes[dtype]))
    if nbytes == 0:
        raise CoreError(f"{prefix}_packed_bytes refuses channels_out {cout}, channels_in {cin}" +
                        (f", kernel {k[0]}" if with_kernel else ""))
    dev = w.device if w.is_cuda else torch.device("cuda", device)
    w = w.detach().to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        packed = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _check(getattr(lib(), prefix + "_pack_weights")(w.data_ptr(), cout, cin, *k, codes[dtype], packed.data_ptr(),
                                                        _current_stream(dev)), prefix + "_pack_weights")
    return packed


def _conv_launch(prefix, entry, args_cls, with_kernel, features, packed, scale, shift, kernel, dilation, residual, relu,
                 out_dtype, canary, stride=None):
    """The call sequence of conv3x3_bn_relu, conv_bn and conv_bn_stride: the entry point `entry` of the C ABI with its
    args class, and `prefix`_packed_bytes for the size of its packed weights.  with_kernel: the entry point has the
    fields `kernel` and `d_residual` (f18); without it the caller passes kernel 3 and no residual (f17).  stride: the
    entry point has the field `stride` and names the extents rows_in, cols_in (f19); the output and the residual then
    have ceil(. / stride) of the features' extents."""
    import torch
    x = features
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4:
        raise CoreError("features must be a device tensor [n][channels_in][rows8][cols8]")
    codes = _head_codes(halves_only=True)
    if x.dtype not in codes:
        raise CoreError(f"features dtype {x.dtype} is neither float16 nor bfloat16 (convert fp32 features first)")
    odt = x.dtype if out_dtype is None else out_dtype
    if odt != x.dtype and odt != torch.float32:
        raise CoreError(f"out_dtype {odt} is neither the features' dtype nor float32")
    same = residual is features
    x = x.contiguous()
    dev = x.device
    n, cin, Hs, Ws = (int(v) for v in x.shape)
    extents = dict(rows8=Hs, cols8=Ws)
    Ho, Wo = Hs, Ws
    if stride is not None:
        if stride not in (1, 2):
            raise CoreError(f"stride {stride} is neither 1 nor 2")
        extents = dict(rows_in=Hs, cols_in=Ws, stride=int(stride))
        Ho, Wo = (Hs + stride - 1) // stride, (Ws + stride - 1) // stride
    sc, sh = _f32_on(scale, dev).reshape(-1), _f32_on(shift, dev).reshape(-1)
    cout = int(sc.numel())
    if int(sh.numel()) != cout:
        raise CoreError(f"scale holds {cout} channels, shift {int(sh.numel())}")
    res = None
    if residual is not None:
        res = x if same else residual
        if not torch.is_tensor(res) or res.device != dev or res.dtype != x.dtype or \
                tuple(int(v) for v in res.shape) != (n, cout, Ho, Wo):
            raise CoreError(f"residual must be a {x.dtype} tensor [{n}][{cout}][{Ho}][{Wo}] on the features' device")
        res = res.contiguous()
    k = (int(kernel),) if with_kernel else ()
    own = dict(kernel=k[0], d_residual=res.data_ptr() if res is not None else None) if with_kernel else {}
    need = int(getattr(lib(), prefix + "_packed_bytes")(cout, cin, *k, codes[x.dtype]))
    if not torch.is_tensor(packed) or packed.device != dev or packed.dtype != torch.uint8 or \
            not packed.is_contiguous() or need == 0 or int(packed.numel()) != need:
        # (the Python packer has the C one's name without "is_")
        raise CoreError(f"packed must be {prefix[3:]}_pack_weights' uint8 tensor for channels_out {cout}, channels_in "
                        f"{cin}{f', kernel {kernel}' if with_kernel else ''} and {x.dtype} on the features' device")
    with torch.cuda.device(dev):
        fresh = _Fresh(dev, canary)
        out = fresh.new("out", (n, cout, Ho, Wo), odt)
        a = args_cls(d_features=x.data_ptr(), dtype=codes[x.dtype], n_images=n, channels_in=cin, channels_out=cout,
                     dilation=int(dilation), d_packed=packed.data_ptr(), d_scale=sc.data_ptr(),
                     d_shift=sh.data_ptr(), relu=int(bool(relu)), d_out=out.data_ptr(),
                     out_dtype=HEAD_F32 if odt == torch.float32 else codes[x.dtype], **extents, **own)
        _check(getattr(lib(), entry)(ctypes.byref(a), _current_stream(dev)), entry)
        if fresh.g:
            return out, fresh.guards()
    return out


def conv3x3_packed_bytes(channels_out, channels_in, dtype):
    """is_conv3x3_packed_bytes: the bytes of the packed weights (0: channels or a dtype code outside the ranges)."""
    return int(lib().is_conv3x3_packed_bytes(int(channels_out), int(channels_in), int(dtype)))


def conv3x3_pack_weights(weight, dtype, device=0):
    """is_conv3x3_pack_weights (instance_stixels_core.h f17): conv.weight [channels_out][channels_in][3][3], a tensor
    or an array, rounded to torch.float16 or torch.bfloat16 and laid out for is_conv3x3_bn_relu.  Returns a uint8
    device tensor of conv3x3_packed_bytes(...) bytes (on the weight's device if it is a device tensor, else on
    cuda:`device`); enqueued on the current torch stream, once per model."""
    return _conv_pack("is_conv3x3", False, weight, dtype, device)


def conv3x3_bn_relu(features, packed, scale, shift, dilation, relu=True, out_dtype=None, canary=0):
    """A dilated 3x3 convolution (padding = dilation, stride 1, no bias) with folded BatchNorm and ReLU of a batch in
    one launch (is_conv3x3_bn_relu, instance_stixels_core.h f17), with the numerics the header fixes.

    features    device tensor [n][channels_in][rows8][cols8], float16 or bfloat16; made contiguous NCHW
    packed      conv3x3_pack_weights(conv.weight, features.dtype) on the same device
    scale, shift   [channels_out] float32, tensors or arrays: the folded BatchNorm (cnn.fold_batchnorm)
    out_dtype   None (the features' dtype) or torch.float32

    Returns the output [n][channels_out][rows8][cols8] on the features' device, enqueued on the current torch stream.
    canary > 0: the output is allocated with that many guard elements in front and behind, filled with a pattern, and
    {"out": (front, back, pattern)} of numpy copies of the guards is returned second (one synchronisation)."""
    return _conv_launch("is_conv3x3", "is_conv3x3_bn_relu", Conv3x3Args, False, features, packed, scale, shift, 3,
                        dilation, None, relu, out_dtype, canary)


def conv_packed_bytes(channels_out, channels_in, kernel, dtype):
    """is_conv_packed_bytes: the bytes of the packed weights (0: channels, a kernel size or a dtype code outside the
    ranges)."""
    return int(lib().is_conv_packed_bytes(int(channels_out), int(channels_in), int(kernel), int(dtype)))


def conv_pack_weights(weight, dtype, device=0):
    """is_conv_pack_weights (instance_stixels_core.h f18): conv.weight [channels_out][channels_in][k][k] with k = 3 or
    1, a tensor or an array, rounded to torch.float16 or torch.bfloat16 and laid out for is_conv_bn.  Returns a uint8
    device tensor of conv_packed_bytes(...) bytes (on the weight's device if it is a device tensor, else on
    cuda:`device`); enqueued on the current torch stream, once per model."""
    return _conv_pack("is_conv", True, weight, dtype, device)


def conv_bn(features, packed, scale, shift, kernel, dilation=1, residual=None, relu=True, out_dtype=None, canary=0):
    """A 3x3 (dilated, padding = dilation) or 1x1 convolution without bias, stride 1, with folded BatchNorm, an
    optional residual added in fp32 between the BatchNorm and the ReLU, and an optional ReLU, of a batch in one launch
    (is_conv_bn, instance_stixels_core.h f18), with the numerics the header fixes.

    features    device tensor [n][channels_in][rows8][cols8], float16 or bfloat16; made contiguous NCHW
    packed      conv_pack_weights(conv.weight, features.dtype) on the same device, of the same `kernel`
    scale, shift   [channels_out] float32, tensors or arrays: the folded BatchNorm (cnn.fold_batchnorm)
    residual    None, or a device tensor [n][channels_out][rows8][cols8] of the features' dtype (it may be `features`)
    out_dtype   None (the features' dtype) or torch.float32

    Returns the output [n][channels_out][rows8][cols8] on the features' device, enqueued on the current torch stream.
    canary > 0: as conv3x3_bn_relu, {"out": (front, back, pattern)} is returned second (one synchronisation)."""
    return _conv_launch("is_conv", "is_conv_bn", ConvBnArgs, True, features, packed, scale, shift, kernel, dilation,
                        residual, relu, out_dtype, canary)


def conv_bn_stride(features, packed, scale, shift, kernel, stride, dilation=1, residual=None, relu=True, out_dtype=None,
                   canary=0):
    """conv_bn with a stride of 1 or 2 (is_conv_bn_stride, instance_stixels_core.h f19): the 3x3 (padding = dilation)
    or 1x1 (no padding) convolution without bias, folded BatchNorm, optional residual and optional ReLU of a batch in
    one launch.  stride 2 needs dilation 1; stride 1 is conv_bn's launch and bytes.

    features    device tensor [n][channels_in][rows_in][cols_in], float16 or bfloat16; made contiguous NCHW
    packed      conv_pack_weights(conv.weight, features.dtype) on the same device, of the same `kernel`
    residual    None, or a device tensor of the features' dtype and the OUTPUT's shape (at stride 1 it may be `features`)

    Returns the output [n][channels_out][ceil(rows_in / stride)][ceil(cols_in / stride)] on the features' device,
    enqueued on the current torch stream.  canary > 0: as conv3x3_bn_relu."""
    return _conv_launch("is_conv", "is_conv_bn_stride", ConvBnStrideArgs, True, features, packed, scale, shift, kernel,
                        dilation, residual, relu, out_dtype, canary, stride=stride)


def stem_packed_bytes(dtype):
    """is_stem_packed_bytes: the bytes of the stem's packed weights (0: a dtype code that is no half)."""
    return int(lib().is_stem_packed_bytes(int(dtype)))


def stem_pack_weights(w0, w1, dtype, device=0):
    """is_stem_pack_weights (instance_stixels_core.h f20): layer0's conv.weight [16][3][7][7] and layer1's
    [16][16][3][3], tensors or arrays, rounded to torch.float16 or torch.bfloat16 and laid out for is_stem.  Returns a
    uint8 device tensor of stem_packed_bytes(...) bytes (on w0's device if it is a device tensor, else on
    cuda:`device`); enqueued on the current torch stream, once per model.  Every refusal is made before a weight goes
    to a device."""
    import torch
    codes = _head_codes(halves_only=True)
    if dtype not in codes:
        raise CoreError(f"dtype {dtype} is neither torch.float16 nor torch.bfloat16")
    ws = [w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, np.float32)) for w in (w0, w1)]
    if tuple(ws[0].shape) != (16, 3, 7, 7) or tuple(ws[1].shape) != (16, 16, 3, 3):
        raise CoreError("w0 must be [16][3][7][7] and w1 [16][16][3][3]")
    dev = ws[0].device if ws[0].is_cuda else device if isinstance(device, torch.device) else torch.device("cuda", device)
    ws = [w.detach().to(device=dev, dtype=torch.float32).contiguous() for w in ws]
    with torch.cuda.device(dev):
        packed = torch.empty((stem_packed_bytes(codes[dtype]),), dtype=torch.uint8, device=dev)
        _check(lib().is_stem_pack_weights(ws[0].data_ptr(), ws[1].data_ptr(), codes[dtype], packed.data_ptr(),
                                          _current_stream(dev)), "is_stem_pack_weights")
    return packed


def stem(image, lut, packed, scale0, shift0, scale1, shift1, want_mid=False, canary=0):
    """The backbone's stem of a batch in one launch (is_stem, instance_stixels_core.h f20): the table look-up of the
    image's bytes, layer0 (7x7, 3 -> 16, folded BatchNorm, ReLU) and layer1 (3x3, 16 -> 16, folded BatchNorm, ReLU),
    with the numerics the header fixes.

    image       device tensor [n][rows][cols][3] uint8; made contiguous
    lut         [3][256] float16 or bfloat16 on the image's device (cnn.input_table): its dtype is the launch's
    packed      stem_pack_weights(w0, w1, lut.dtype) on the same device
    scale0 .. shift1   [16] float32 each, tensors or arrays: the folded BatchNorms (cnn.fold_batchnorm)

    Returns layer1's output [n][16][rows][cols] of the table's dtype on the image's device, enqueued on the current
    torch stream; with want_mid (out, mid), layer0's output in the same shape.  canary > 0: the outputs are allocated
    with that many guard elements in front and behind, filled with a pattern, and {"out": (front, back, pattern)[,
    "mid": ...]} of numpy copies of the guards is returned last (one synchronisation)."""
    import torch
    if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 4 or \
            int(image.shape[3]) != 3:
        raise CoreError("image must be a uint8 device tensor [n][rows][cols][3]")
    dev = image.device
    codes = _head_codes(halves_only=True)
    if not torch.is_tensor(lut) or lut.device != dev or lut.dtype not in codes or tuple(lut.shape) != (3, 256):
        raise CoreError("lut must be a float16 or bfloat16 tensor [3][256] on the image's device")
    dtype = lut.dtype
    if not torch.is_tensor(packed) or packed.device != dev or packed.dtype != torch.uint8 or \
            not packed.is_contiguous() or int(packed.numel()) != stem_packed_bytes(codes[dtype]):
        raise CoreError(f"packed must be stem_pack_weights' uint8 tensor for {dtype} on the image's device")
    folds = [_f32_on(v, dev).reshape(-1) for v in (scale0, shift0, scale1, shift1)]
    if any(int(f.numel()) != 16 for f in folds):
        raise CoreError("scale0, shift0, scale1 and shift1 must hold 16 channels each")
    x, table = image.contiguous(), lut.contiguous()
    n, H, W = (int(v) for v in x.shape[:3])
    with torch.cuda.device(dev):
        fresh = _Fresh(dev, canary)
        ret, ptr = fresh.rows((("out", True, (n, 16, H, W), dtype), ("mid", want_mid, (n, 16, H, W), dtype)))
        a = StemArgs(d_image=x.data_ptr(), n_images=n, rows=H, cols=W, d_lut=table.data_ptr(), dtype=codes[dtype],
                     d_packed=packed.data_ptr(), d_scale0=folds[0].data_ptr(), d_shift0=folds[1].data_ptr(),
                     d_scale1=folds[2].data_ptr(), d_shift1=folds[3].data_ptr(), d_mid=ptr["mid"], d_out=ptr["out"])
        _check(lib().is_stem(ctypes.byref(a), _current_stream(dev)), "is_stem")
        ret = tuple(ret.values())
        if fresh.g:
            ret = ret + (fresh.guards(),)
    return ret if len(ret) > 1 else ret[0]


def segmentation_head_backward_scratch_bytes(n_images, K, rows8, cols8, channels):
    """is_segmentation_head_backward_scratch_bytes: the scratch a call of that shape needs (0: a refused shape)."""
    return int(lib().is_segmentation_head_backward_scratch_bytes(int(n_images), int(K), int(rows8), int(cols8),
                                                                 int(channels)))


def segmentation_head_backward(features, weight, cnn_out, grad_out, n_classes, want_features=True, want_weight=True,
                               want_bias=True, want_logits=False, canary=0):
    """The backward pass of the segmentation head (is_segmentation_head_backward, instance_stixels_core.h f14).

    features    device tensor [n][K][rows8][cols8], float32, float16 or bfloat16 (made contiguous)
    weight      [channels][K] (or [channels][K][1][1]) float32
    cnn_out     device float32 [n][channels][rows8][cols8]: the float output of core.segmentation_head, saved
    grad_out    device float32 [n][channels][rows8][cols8]: the gradient with respect to cnn_out; read in place when
                each frame's planes are contiguous (a batch stride above channels * rows8 * cols8 is allowed)

    Returns a dict with the requested ones of "features" (the features' shape and dtype), "weight" [channels][K],
    "bias" [channels] and "logits" [n][channels][rows8][cols8] (float32), on the features' device, enqueued on the
    current torch stream; the scratch is allocated here.  canary > 0: every output and the scratch get that many guard
    elements in front and behind, and the dict has "guards": {name: (front, back, pattern)} (one synchronisation)."""
    import torch
    x = features
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4:
        raise CoreError("features must be a device tensor [n][K][rows8][cols8]")
    codes = _head_codes()
    if x.dtype not in codes:
        raise CoreError(f"features dtype {x.dtype} is none of float32, float16, bfloat16")
    x = x.detach().contiguous()
    dev = x.device
    n, K, Hs, Ws = x.shape
    w = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    CH = int(w.shape[0])
    w = w.reshape(CH, -1)
    if w.shape[1] != K:
        raise CoreError(f"weight holds {w.shape[1]} values per channel, the features have K = {K}")
    shape = (n, CH, Hs, Ws)
    y = cnn_out
    if y.device != dev or y.dtype != torch.float32 or tuple(y.shape) != shape:
        raise CoreError(f"cnn_out must be a float32 tensor {shape} on the features' device")
    y = y.detach().contiguous()
    gy = grad_out
    if gy.device != dev or gy.dtype != torch.float32 or tuple(gy.shape) != shape:
        raise CoreError(f"grad_out must be a float32 tensor {shape} on the features' device")
    gy, gy_stride = _frame_planes(gy.detach(), CH)
    if not (want_features or want_weight or want_bias or want_logits):
        raise CoreError("no gradient is asked for")
    with torch.cuda.device(dev):
        nbytes = _scratch_or_raise(segmentation_head_backward_scratch_bytes,
                                   dict(n_images=n, K=K, rows8=Hs, cols8=Ws, channels=CH))
        fresh = _Fresh(dev, canary)
        out, ptr = fresh.rows((("features", want_features, (n, K, Hs, Ws), x.dtype),
                               ("weight", want_weight, (CH, K), torch.float32),
                               ("bias", want_bias, (CH,), torch.float32),
                               ("logits", want_logits, shape, torch.float32)))
        scratch = fresh.scratch(nbytes)
        a = SegmentationHeadBackwardArgs(
            d_features=x.data_ptr(), dtype=codes[x.dtype], n_images=n, K=K, rows8=Hs, cols8=Ws, d_weight=w.data_ptr(),
            n_classes=int(n_classes), n_regression=CH - int(n_classes), d_cnn_out=y.data_ptr(),
            d_grad_out=gy.data_ptr(), grad_image_stride=gy_stride, d_grad_features=ptr["features"],
            d_grad_weight=ptr["weight"], d_grad_bias=ptr["bias"], d_grad_logits=ptr["logits"],
            d_scratch=scratch.data_ptr(), scratch_bytes=nbytes)
        _check(lib().is_segmentation_head_backward(ctypes.byref(a), _current_stream(dev)),
               "is_segmentation_head_backward")
        if fresh.g:
            out["guards"] = fresh.guards()
    return out


def conv_bn_backward_scratch_bytes(n_images, channels_in, channels_out, rows8, cols8, kernel, dtype):
    """is_conv_bn_backward_scratch_bytes: the scratch a call of that shape needs (0: a refused shape)."""
    return int(lib().is_conv_bn_backward_scratch_bytes(int(n_images), int(channels_in), int(channels_out), int(rows8),
                                                       int(cols8), int(kernel), int(dtype)))


def conv_bn_backward(features, weight, scale, out, grad_out, kernel, dilation=1, relu=True, want_features=True,
                     want_weight=True, want_scale=True, want_shift=True, want_pre=False, features_add=None,
                     grad_features_dtype=None, canary=0):
    """The backward pass of conv_bn at stride 1 with BatchNorm frozen at its running statistics (is_conv_bn_backward,
    instance_stixels_core.h f21), with the numerics the header fixes.

    features    device tensor [n][channels_in][rows8][cols8], float16 or bfloat16 (made contiguous)
    weight      conv.weight [channels_out][channels_in][kernel][kernel] float32 (the master weight, not the pack)
    scale       [channels_out] float32: the folded BatchNorm scale the forward ran with
    out         the forward's saved output [n][channels_out][rows8][cols8], the features' dtype or float32; read with
                relu only (it may be None without)
    grad_out    the gradient with respect to `out`, the features' dtype or float32; read in place when each frame's
                planes are contiguous (a batch stride above channels_out * rows8 * cols8 is allowed)
    features_add   None, or a tensor of the features' shape and dtype that is added to "features" in fp32 before its
                single rounding (the other gradient path into a block's input)
    grad_features_dtype   None (the features' dtype) or torch.float32

    Returns a dict with the requested ones of "features", "weight" (conv.weight's shape), "scale", "shift"
    [channels_out] (float32) and "pre" [n][channels_out][rows8][cols8] (the features' dtype: the masked gradient, which
    is the gradient with respect to the forward's residual operand), on the features' device, enqueued on the current
    torch stream; the scratch is allocated here.  canary > 0: every output and the scratch get that many guard
    elements in front and behind, and the dict has "guards": {name: (front, back, pattern)} (one synchronisation)."""
    return _conv_backward(None, features, weight, scale, out, grad_out, kernel, dilation, relu, want_features, want_weight,
                          want_scale, want_shift, want_pre, features_add, grad_features_dtype, canary)


def conv_bn_stride_backward_scratch_bytes(n_images, channels_in, channels_out, rows_in, cols_in, kernel, stride, dtype):
    """is_conv_bn_stride_backward_scratch_bytes: the scratch a call of that shape needs (0: a refused shape)."""
    return int(lib().is_conv_bn_stride_backward_scratch_bytes(int(n_images), int(channels_in), int(channels_out),
                                                              int(rows_in), int(cols_in), int(kernel), int(stride),
                                                              int(dtype)))


def conv_bn_stride_backward(features, weight, scale, out, grad_out, kernel, stride, dilation=1, relu=True,
                            want_features=True, want_weight=True, want_scale=True, want_shift=True, want_pre=False,
                            features_add=None, grad_features_dtype=None, canary=0):
    """conv_bn_backward with a stride of 1 or 2 (is_conv_bn_stride_backward, instance_stixels_core.h f22): the backward
    pass of conv_bn_stride.  Arguments and result as conv_bn_backward, except that `features`, "features" and
    `features_add` have the INPUT's extents [n][channels_in][rows_in][cols_in] and `out`, `grad_out` and "pre" the
    OUTPUT's, ceil(rows_in / stride) x ceil(cols_in / stride).  At stride 1 the bytes are conv_bn_backward's; stride 2
    needs dilation 1, and "features" needs channels_in % 32 == 0 (layer2's 16 channels get weight, scale and shift
    only)."""
    return _conv_backward(stride, features, weight, scale, out, grad_out, kernel, dilation, relu, want_features,
                          want_weight, want_scale, want_shift, want_pre, features_add, grad_features_dtype, canary)


def _conv_backward(stride, features, weight, scale, out, grad_out, kernel, dilation, relu, want_features, want_weight,
                   want_scale, want_shift, want_pre, features_add, grad_features_dtype, canary):
    """The call sequence of conv_bn_backward (stride None: is_conv_bn_backward, extents rows8 / cols8) and
    conv_bn_stride_backward (is_conv_bn_stride_backward, extents rows_in / cols_in)."""
    ext = ("rows8", "cols8") if stride is None else ("rows_in", "cols_in")
    import torch
    x = features
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4:
        raise CoreError(f"features must be a device tensor [n][channels_in][{ext[0]}][{ext[1]}]")
    codes = _head_codes(halves_only=True)
    if x.dtype not in codes:
        raise CoreError(f"features dtype {x.dtype} is neither float16 nor bfloat16 (fp32 features are not built)")
    x = x.detach().contiguous()
    dev = x.device
    n, cin, Hs, Ws = (int(v) for v in x.shape)
    k = int(kernel)
    w = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    if w.dim() != 4 or int(w.shape[1]) != cin or tuple(int(v) for v in w.shape[2:]) != (k, k):
        raise CoreError(f"weight must be [channels_out][{cin}][{k}][{k}]")
    cout = int(w.shape[0])
    sc = _f32_on(scale, dev).reshape(-1)
    if int(sc.numel()) != cout:
        raise CoreError(f"scale holds {int(sc.numel())} channels, the weight {cout}")
    st = 1 if stride is None else int(stride)
    if st not in (1, 2):
        raise CoreError(f"stride {stride} is neither 1 nor 2")
    shape = (n, cout, (Hs + st - 1) // st, (Ws + st - 1) // st)      # the OUTPUT's: out, grad_out, "pre"

    def half_or_f32(t, name):
        if not torch.is_tensor(t) or t.device != dev or t.dtype not in (x.dtype, torch.float32) or \
                tuple(int(v) for v in t.shape) != shape:
            raise CoreError(f"{name} must be a {x.dtype} or float32 tensor {shape} on the features' device")
        return HEAD_F32 if t.dtype == torch.float32 else codes[x.dtype]

    y, y_code = None, codes[x.dtype]
    if relu:
        y_code = half_or_f32(out, "out")
        y = out.detach().contiguous()
    gy_code = half_or_f32(grad_out, "grad_out")
    gy, gy_stride = _frame_planes(grad_out.detach(), cout)
    xdt = x.dtype if grad_features_dtype is None else grad_features_dtype
    if xdt != x.dtype and xdt != torch.float32:
        raise CoreError(f"grad_features_dtype {xdt} is neither the features' dtype nor float32")
    add = None
    if features_add is not None:
        if not want_features:
            raise CoreError("features_add without want_features")
        add = features_add
        if not torch.is_tensor(add) or add.device != dev or add.dtype != x.dtype or tuple(add.shape) != tuple(x.shape):
            raise CoreError(f"features_add must be a {x.dtype} tensor of the features' shape on their device")
        add = add.detach().contiguous()
    if not (want_features or want_weight or want_scale or want_shift or want_pre):
        raise CoreError("no gradient is asked for")
    with torch.cuda.device(dev):
        extents = {ext[0]: Hs, ext[1]: Ws}
        nbytes = _scratch_or_raise(conv_bn_backward_scratch_bytes if stride is None else
                                   conv_bn_stride_backward_scratch_bytes,
                                   dict(n_images=n, channels_in=cin, channels_out=cout, **extents, kernel=k,
                                        **({} if stride is None else dict(stride=st))),
                                   dtype=codes[x.dtype])
        fresh = _Fresh(dev, canary)
        ret, ptr = fresh.rows((("features", want_features, (n, cin, Hs, Ws), xdt),
                               ("weight", want_weight, (cout, cin, k, k), torch.float32),
                               ("scale", want_scale, (cout,), torch.float32),
                               ("shift", want_shift, (cout,), torch.float32),
                               ("pre", want_pre, shape, x.dtype)))
        scratch = fresh.scratch(nbytes)
        a = (ConvBnBackwardArgs if stride is None else ConvBnStrideBackwardArgs)(
            d_features=x.data_ptr(), dtype=codes[x.dtype], n_images=n, channels_in=cin, channels_out=cout, **extents,
            kernel=k, dilation=int(dilation), **({} if stride is None else dict(stride=st)), d_weight=w.data_ptr(),
            d_scale=sc.data_ptr(),
            d_out=y.data_ptr() if y is not None else None, out_dtype=y_code, relu=int(bool(relu)),
            d_grad_out=gy.data_ptr(), grad_out_dtype=gy_code, grad_image_stride=gy_stride,
            d_grad_features=ptr["features"], grad_features_dtype=HEAD_F32 if xdt == torch.float32 else codes[x.dtype],
            d_grad_features_add=add.data_ptr() if add is not None else None, d_grad_weight=ptr["weight"],
            d_grad_scale=ptr["scale"], d_grad_shift=ptr["shift"], d_grad_pre=ptr["pre"],
            d_scratch=scratch.data_ptr(), scratch_bytes=nbytes)
        entry = "is_conv_bn_backward" if stride is None else "is_conv_bn_stride_backward"
        _check(getattr(lib(), entry)(ctypes.byref(a), _current_stream(dev)), entry)
        if fresh.g:
            ret["guards"] = fresh.guards()
    return ret


def stem_backward_scratch_bytes(n_images, rows, cols, channels_next, dtype):
    """is_stem_backward_scratch_bytes: the scratch a call of that shape needs (0: a refused shape)."""
    return int(lib().is_stem_backward_scratch_bytes(int(n_images), int(rows), int(cols), int(channels_next), int(dtype)))


_STEM_BACKWARD_OUTPUTS = ("weight0", "scale0", "shift0", "weight1", "scale1", "shift1")


def stem_backward(image, lut, w0, w1, scale0, scale1, mid, out, grad_out=None, grad_next=None, weight_next=None,
                  scale_next=None, want_weight0=True, want_scale0=True, want_shift0=True, want_weight1=True,
                  want_scale1=True, want_shift1=True, want_pre=False, canary=0):
    """The backward pass of `stem` with BatchNorm frozen (is_stem_backward, instance_stixels_core.h f23), with the
    numerics the header fixes.

    image, lut  as `stem` takes them; the table's dtype is the launch's
    w0, w1      layer0's conv.weight [16][3][7][7] and layer1's [16][16][3][3], float32: the master weights, not the pack
    scale0, scale1   [16] float32 each: the folded BatchNorm scales the forward ran with
    mid, out    the forward's saved tensors (stem(..., want_mid=True)), [n][16][rows][cols] of the table's dtype
    grad_out    the gradient with respect to `out`, the table's dtype or float32; read in place when each frame's planes
                are contiguous
    grad_next, weight_next, scale_next   the other gradient source, in place of grad_out: the masked gradient of the
                stride-2 3x3 layer that reads `out` (conv_bn_stride_backward's "pre" of layer2), [n][channels_next]
                [(rows + 1) / 2][(cols + 1) / 2] of the table's dtype, with that layer's conv.weight [channels_next][16]
                [3][3] float32 and folded scale [channels_next]

    Returns a dict with the requested ones of "weight0", "scale0", "shift0", "weight1", "scale1", "shift1" (float32,
    the parameters' shapes) and, with want_pre, "pre0" and "pre1" [n][16][rows][cols] of the table's dtype (the masked
    gradients behind layer0's and layer1's ReLU), on the image's device, enqueued on the current torch stream; the
    scratch is allocated here.  canary > 0: every output and the scratch get that many guard elements in front and
    behind, and the dict has "guards": {name: (front, back, pattern)} (one synchronisation).  Every refusal is made
    before anything is allocated on the device."""
    import torch
    source_b = grad_next is not None or weight_next is not None or scale_next is not None
    if grad_out is not None and source_b:
        raise CoreError("both gradient sources: grad_out and grad_next's arguments")
    if grad_out is None and not source_b:
        raise CoreError("no gradient source: grad_out and grad_next are None")
    if source_b and (grad_next is None or weight_next is None or scale_next is None):
        raise CoreError("grad_next, weight_next and scale_next come together")
    if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 4 or \
            int(image.shape[3]) != 3:
        raise CoreError("image must be a uint8 device tensor [n][rows][cols][3]")
    dev = image.device
    codes = _head_codes(halves_only=True)
    if not torch.is_tensor(lut) or lut.device != dev or lut.dtype not in codes or tuple(lut.shape) != (3, 256):
        raise CoreError("lut must be a float16 or bfloat16 tensor [3][256] on the image's device")
    dtype = lut.dtype
    n, H, W = (int(v) for v in image.shape[:3])
    shape = (n, 16, H, W)
    for name, t in (("mid", mid), ("out", out)):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or tuple(int(v) for v in t.shape) != shape:
            raise CoreError(f"{name} must be a {dtype} tensor {shape} on the image's device")
    cn = 0
    if source_b:
        if not torch.is_tensor(grad_next) or grad_next.device != dev or grad_next.dtype != dtype or grad_next.dim() != 4 or \
                (int(grad_next.shape[0]), int(grad_next.shape[2]), int(grad_next.shape[3])) != (n, (H + 1) // 2, (W + 1) // 2):
            raise CoreError(f"grad_next must be a {dtype} tensor [{n}][channels_next][{(H + 1) // 2}][{(W + 1) // 2}] on "
                            "the image's device")
        cn = int(grad_next.shape[1])
        if cn % 32 or not 32 <= cn <= 128:
            raise CoreError(f"channels_next {cn} is no multiple of 32 in [32, 128]")
        wn = weight_next if torch.is_tensor(weight_next) else torch.from_numpy(np.ascontiguousarray(weight_next, np.float32))
        sn = scale_next if torch.is_tensor(scale_next) else torch.tensor(np.asarray(scale_next, np.float32))
        if tuple(wn.shape) != (cn, 16, 3, 3) or int(sn.numel()) != cn:
            raise CoreError(f"weight_next must be [{cn}][16][3][3] and scale_next hold {cn} channels")
    elif not torch.is_tensor(grad_out) or grad_out.device != dev or grad_out.dtype not in (dtype, torch.float32) or \
            tuple(int(v) for v in grad_out.shape) != shape:
        raise CoreError(f"grad_out must be a {dtype} or float32 tensor {shape} on the image's device")
    ws = [w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, np.float32)) for w in (w0, w1)]
    if tuple(ws[0].shape) != (16, 3, 7, 7) or tuple(ws[1].shape) != (16, 16, 3, 3):
        raise CoreError("w0 must be [16][3][7][7] and w1 [16][16][3][3]")
    scales = [v if torch.is_tensor(v) else torch.tensor(np.asarray(v, np.float32)) for v in (scale0, scale1)]
    if any(int(s.numel()) != 16 for s in scales):
        raise CoreError("scale0 and scale1 must hold 16 channels each")
    wants = dict(zip(_STEM_BACKWARD_OUTPUTS, (want_weight0, want_scale0, want_shift0, want_weight1, want_scale1,
                                              want_shift1)))
    if not (any(wants.values()) or want_pre):
        raise CoreError("no gradient is asked for")
    ws = [w.detach().to(device=dev, dtype=torch.float32).contiguous() for w in ws]
    scales = [_f32_on(s, dev).reshape(-1) for s in scales]
    x, table, m, y = image.contiguous(), lut.contiguous(), mid.detach().contiguous(), out.detach().contiguous()
    source = {}
    if source_b:
        gn = grad_next.detach().contiguous()
        wn = wn.detach().to(device=dev, dtype=torch.float32).contiguous()
        sn = _f32_on(sn, dev).reshape(-1)
        source = dict(d_grad_next=gn.data_ptr(), channels_next=cn, d_weight_next=wn.data_ptr(), d_scale_next=sn.data_ptr())
    else:
        gy, gy_stride = _frame_planes(grad_out.detach(), 16)
        source = dict(d_grad_out=gy.data_ptr(), grad_image_stride=gy_stride,
                      grad_out_dtype=HEAD_F32 if grad_out.dtype == torch.float32 else codes[dtype])
    with torch.cuda.device(dev):
        nbytes = _scratch_or_raise(stem_backward_scratch_bytes, dict(n_images=n, rows=H, cols=W, channels_next=cn),
                                   dtype=codes[dtype])
        views = {"weight0": (16, 3, 7, 7), "scale0": (16,), "shift0": (16,), "weight1": (16, 16, 3, 3), "scale1": (16,),
                 "shift1": (16,)}
        fresh = _Fresh(dev, canary)
        ret, ptr = fresh.rows([(name, wants[name], view, torch.float32) for name, view in views.items()] +
                              [(name, want_pre, shape, dtype) for name in ("pre0", "pre1")])
        scratch = fresh.scratch(nbytes)
        a = StemBackwardArgs(
            d_image=x.data_ptr(), n_images=n, rows=H, cols=W, d_lut=table.data_ptr(), dtype=codes[dtype],
            d_w0=ws[0].data_ptr(), d_w1=ws[1].data_ptr(), d_scale0=scales[0].data_ptr(), d_scale1=scales[1].data_ptr(),
            d_mid=m.data_ptr(), d_out=y.data_ptr(), **source, d_grad_weight0=ptr["weight0"], d_grad_scale0=ptr["scale0"],
            d_grad_shift0=ptr["shift0"], d_grad_weight1=ptr["weight1"], d_grad_scale1=ptr["scale1"],
            d_grad_shift1=ptr["shift1"], d_grad_pre1=ptr["pre1"], d_grad_pre0=ptr["pre0"], d_scratch=scratch.data_ptr(),
            scratch_bytes=nbytes)
        _check(lib().is_stem_backward(ctypes.byref(a), _current_stream(dev)), "is_stem_backward")
        if fresh.g:
            ret["guards"] = fresh.guards()
    return ret


def semantic_nll_scratch_bytes(n_images, rows8, cols8):
    """is_semantic_nll_scratch_bytes: the scratch a call of that shape needs (0: a refused shape)."""
    return int(lib().is_semantic_nll_scratch_bytes(int(n_images), int(rows8), int(cols8)))


def _semantic_nll(entry, args_cls, scratch_fn, scratch_more, count, target_fields, cnn_out, n_classes, ignore_index,
                  grad, check, canary):
    """The call sequence of semantic_nll and semantic_nll_up: the entry point `entry` of the C ABI with its args class
    and the scratch of scratch_fn(n_images, rows8, cols8, **scratch_more).  count: the torch dtype of valid_count
    and bad_count.  target_fields(n, rows8, cols8, dev) checks the caller's target and returns the tensor to pass and
    the args fields that are the entry point's own."""
    import torch
    y = cnn_out
    if not torch.is_tensor(y) or not y.is_cuda or y.dtype != torch.float32 or y.dim() != 4 or y.shape[1] < n_classes:
        raise CoreError("cnn_out must be a device float32 tensor [n][C >= n_classes][rows8][cols8]")
    dev = y.device
    n, _, Hs, Ws = y.shape
    y, y_stride = _frame_planes(y.detach(), n_classes)
    t, own = target_fields(n, Hs, Ws, dev)
    with torch.cuda.device(dev):
        nbytes = _scratch_or_raise(scratch_fn, dict(n_images=n, rows8=Hs, cols8=Ws, **scratch_more))
        fresh = _Fresh(dev, canary)
        loss = fresh.new("loss", (1,), torch.float32)
        valid, bad = fresh.new("valid_count", (1,), count), fresh.new("bad_count", (1,), count)
        gr, g_stride = None, 0
        if torch.is_tensor(grad):
            gr = grad
            if gr.device != dev or gr.dtype != torch.float32 or gr.dim() != 4 or gr.shape[0] != n or \
                    gr.shape[1] < n_classes or tuple(gr.shape[2:]) != (Hs, Ws) or not _planes_in_place(gr, n_classes):
                raise CoreError("grad must be a device float32 tensor [n][C' >= n_classes][rows8][cols8] whose "
                                "planes are contiguous")
            g_stride = gr.stride(0) if n > 1 else n_classes * Hs * Ws
        elif grad:
            gr, g_stride = fresh.new("grad", (n, n_classes, Hs, Ws), torch.float32), n_classes * Hs * Ws
        scratch = fresh.scratch(nbytes)
        a = args_cls(d_cnn_out=y.data_ptr(), cnn_image_stride=y_stride, d_target=t.data_ptr(),
                     ignore_index=int(ignore_index), n_images=n, rows8=Hs, cols8=Ws, n_classes=int(n_classes),
                     d_loss=loss.data_ptr(), d_valid_count=valid.data_ptr(), d_bad_count=bad.data_ptr(),
                     d_grad=gr.data_ptr() if gr is not None else None, grad_image_stride=g_stride,
                     d_scratch=scratch.data_ptr(), scratch_bytes=nbytes, **own)
        _check(getattr(lib(), entry)(ctypes.byref(a), _current_stream(dev)), entry)
        if check:
            nb = int(bad.item())
            if nb:
                raise CoreError(f"{nb} targets are neither a class in [0, {int(n_classes)}) nor ignore_index "
                                f"{int(ignore_index)}")
        out = (loss, valid, bad, gr)
        if fresh.g:
            out = out + (fresh.guards(),)
    return out


def semantic_nll(cnn_out, target, n_classes, ignore_index=255, grad=True, check=True, canary=0):
    """nn.NLLLoss(reduction='mean', ignore_index) on the class planes of the head's float output, with its gradient
    (is_semantic_nll, instance_stixels_core.h f14).

    cnn_out     device float32 [n][C >= n_classes][rows8][cols8]; read in place when each frame's planes are contiguous
    target      device uint8 or int32 [n][rows8][cols8] (what core.mode_downsample writes for the semantic labels)
    grad        True: a new float32 tensor [n][n_classes][rows8][cols8]; a device float32 tensor [n][C'][rows8][cols8]
                with C' >= n_classes and contiguous planes: its first n_classes planes are written in place (the
                regression planes are left to core.offset_loss); False: no gradient

    Returns (loss [1] float32, valid_count [1] int32, bad_count [1] int32, grad or None) on cnn_out's device, enqueued
    on the current torch stream.  check=True reads bad_count back (one synchronisation) and raises CoreError when a
    target is neither a class nor ignore_index.  canary > 0: fresh outputs and the scratch get guards, returned as a
    dict {name: (front, back, pattern)} in fifth place."""
    import torch

    def target_fields(n, Hs, Ws, dev):
        dtypes = {torch.uint8: DTYPE_UINT8, torch.int32: DTYPE_INT32}
        if target.device != dev or target.dtype not in dtypes or tuple(target.shape) != (n, Hs, Ws):
            raise CoreError(f"target must be a uint8 or int32 tensor {(n, Hs, Ws)} on cnn_out's device")
        return target.contiguous(), dict(target_dtype=dtypes[target.dtype])
    return _semantic_nll("is_semantic_nll", SemanticNllArgs, semantic_nll_scratch_bytes, {}, torch.int32, target_fields,
                         cnn_out, n_classes, ignore_index, grad, check, canary)


def semantic_nll_up_scratch_bytes(n_images, rows8, cols8, n_classes):
    """is_semantic_nll_up_scratch_bytes: the scratch a call of that shape needs (0: a refused shape)."""
    return int(lib().is_semantic_nll_up_scratch_bytes(int(n_images), int(rows8), int(cols8), int(n_classes)))


def semantic_nll_up(cnn_out, target_full, n_classes, ignore_index=255, grad=True, check=True, canary=0):
    """The classification loss of the reference's full-resolution models on the head's float output:
    nn.NLLLoss(reduction='mean', ignore_index)(log_softmax(up(.))) with the fixed bilinear `up` layer, and its gradient
    with respect to the class planes (is_semantic_nll_up, instance_stixels_core.h f16).

    cnn_out     device float32 [n][C >= n_classes][rows8][cols8]; read in place when each frame's planes are contiguous
    target_full device uint8 [n][8 * rows8][cols], cols >= 8 * cols8: class ids at full resolution (the pixels right
                of 8 * cols8 take no part)
    grad        True: a new float32 tensor [n][n_classes][rows8][cols8]; a device float32 tensor [n][C'][rows8][cols8]
                with C' >= n_classes and contiguous planes: its first n_classes planes are written in place (the
                regression planes are left to core.offset_loss); False: the loss alone, no residual is computed

    Returns (loss [1] float32, valid_count [1] int64, bad_count [1] int64, grad or None) on cnn_out's device, enqueued
    on the current torch stream.  check=True reads bad_count back (one synchronisation) and raises CoreError when a
    target is neither a class nor ignore_index.  canary > 0: fresh outputs and the scratch get guards, returned as a
    dict {name: (front, back, pattern)} in fifth place."""
    import torch

    def target_fields(n, Hs, Ws, dev):
        t = target_full
        if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.uint8 or t.dim() != 3 or \
                tuple(t.shape[:2]) != (n, 8 * Hs) or t.shape[2] < 8 * Ws:
            raise CoreError(f"target_full must be a uint8 tensor {(n, 8 * Hs)} x (cols >= {8 * Ws}) on cnn_out's device")
        return t.contiguous(), dict(mode=CNN_UP_DECONV, rows=8 * Hs, cols=int(t.shape[2]))
    return _semantic_nll("is_semantic_nll_up", SemanticNllUpArgs, semantic_nll_up_scratch_bytes,
                         dict(n_classes=int(n_classes)), torch.int64, target_fields, cnn_out, n_classes, ignore_index,
                         grad, check, canary)


def cnn_label_maps_ptr(stream=0, class_to_label=None, **fields):
    """is_cnn_label_maps on raw device pointers (ints): fields are those of CnnLabelArgs; class_to_label: a host
    sequence of n_classes label values, None for Cityscapes trainId -> labelId.  Asynchronous on `stream`; returns the
    return code and raises nothing (the tests check IS_EINVAL)."""
    a = _with_reserved(CnnLabelArgs, fields)
    table = None
    if class_to_label is not None:
        table = np.ascontiguousarray(class_to_label, np.uint8)
        a.h_class_to_label = table.ctypes.data
    return lib().is_cnn_label_maps(ctypes.byref(a), ctypes.c_void_p(int(stream)))


def cnn_label_maps(cnn_out, n_classes, mode="nearest", cols=None, gt_label=None, n_labels=CITYSCAPES_N_LABELS,
                   confusion=None, want_label=True, want_class8=False, class_to_label=None, canary=0, stream=0):
    """The CNN's own label image of a batch at full resolution and its confusion table in one launch
    (is_cnn_label_maps, instance_stixels_core.h f15).

    cnn_out     device float32 [n][channels >= n_classes][rows8][cols8]: the float output of core.segmentation_head
                (costs: the arg-min is the class); made contiguous
    mode        "nearest" (each cell's class in its 8 x 8 pixels) or "deconv" (the reference's fixed bilinear
                transposed convolution of the planes, then the arg-min per pixel)
    cols        the image width, >= 8 * cols8 (the default); the pixels right of 8 * cols8 are 0 and are not scored
    gt_label    device uint8 [n][8 * rows8][cols]: with it the confusion table [n_labels][n_labels] (int64 on the
                device, gt x pred; n_labels defaults to the 34 Cityscapes labelIds) is ADDED to `confusion` (a device
                int64 tensor of that shape), or to a new zero table; what evaluation.cityscapes_iou takes
    class_to_label   a host sequence of n_classes label values; None: Cityscapes trainId -> labelId

    Returns a dict with the requested ones of "label" (uint8 [n][8 * rows8][cols]), "class8" (uint8 [n][rows8][cols8])
    and "confusion", on cnn_out's device, enqueued on `stream` or else the current torch stream.  canary > 0: fresh
    outputs get that many guard elements in front and behind, and the dict has "guards": {name: (front, back,
    pattern)} (one synchronisation)."""
    import torch
    y = cnn_out
    if not torch.is_tensor(y) or not y.is_cuda or y.dtype != torch.float32 or y.dim() != 4:
        raise CoreError("cnn_out must be a device float32 tensor [n][channels][rows8][cols8]")
    if mode not in CNN_UP_MODES:
        raise CoreError(f"mode {mode!r} is neither 'nearest' nor 'deconv'")
    y = y.detach().contiguous()
    dev = y.device
    n, CH, Hs, Ws = y.shape
    rows = 8 * Hs
    cols = 8 * Ws if cols is None else int(cols)
    if cols < 8 * Ws:
        raise CoreError(f"cols {cols} is below 8 * cols8 = {8 * Ws}")
    if confusion is not None and gt_label is None:
        raise CoreError("a confusion table needs gt_label")
    if not (want_label or want_class8 or gt_label is not None):
        raise CoreError("no output is asked for")
    table = None if class_to_label is None else np.ascontiguousarray(class_to_label, np.uint8)
    if table is not None and table.size != int(n_classes):
        raise CoreError(f"class_to_label holds {table.size} values, n_classes is {int(n_classes)}")
    with torch.cuda.device(dev):
        fresh = _Fresh(dev, canary)
        out, ptr = fresh.rows((("label", want_label, (n, rows, cols), torch.uint8),
                               ("class8", want_class8, (n, Hs, Ws), torch.uint8)))
        gt = conf = None
        if gt_label is not None:
            gt, nl = gt_label, int(n_labels)
            if not torch.is_tensor(gt) or gt.device != dev or gt.dtype != torch.uint8 or \
                    tuple(gt.shape) != (n, rows, cols):
                raise CoreError(f"gt_label must be a uint8 tensor {(n, rows, cols)} on cnn_out's device")
            gt = gt.contiguous()
            if confusion is None:
                conf = fresh.new("confusion", (nl, nl), torch.int64).zero_()   # (the table is added to)
            else:
                conf = confusion
                if not torch.is_tensor(conf) or conf.device != dev or conf.dtype != torch.int64 or \
                        tuple(conf.shape) != (nl, nl) or not conf.is_contiguous():
                    raise CoreError(f"confusion must be a contiguous int64 tensor {(nl, nl)} on cnn_out's device")
            out["confusion"] = conf
        a = CnnLabelArgs(d_cnn_out=y.data_ptr(), n_images=n, channels=CH, n_classes=int(n_classes), rows8=Hs, cols8=Ws,
                         mode=CNN_UP_MODES[mode], rows=rows, cols=cols,
                         h_class_to_label=table.ctypes.data if table is not None else None,
                         d_class8=ptr["class8"], d_label=ptr["label"],
                         d_gt_label=gt.data_ptr() if gt is not None else None,
                         n_labels=int(n_labels) if gt is not None else 0,
                         d_confusion=conf.data_ptr() if conf is not None else None)
        s = ctypes.c_void_p(int(stream)) if stream else _current_stream(dev)
        _check(lib().is_cnn_label_maps(ctypes.byref(a), s), "is_cnn_label_maps")
        if fresh.g:
            out["guards"] = fresh.guards()
    return out
