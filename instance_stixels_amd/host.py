"""Python view of the C++ `Stixels` host class (instance_stixels_amd/host/Stixels.cpp).

Method names, argument meaning and call order are those of the reference's class
(/root/reference/InstanceStixels/include/InstanceStixels/Stixels.hpp:40-96) so that tests read
like its callers (apps/run_cityscapes.cu:328-449).  Everything executes in the C++ library; this
module only marshals numpy arrays.
"""
import ctypes
import dataclasses
import os

import numpy as np

from . import core as _core
from .config import StixelConfig, StixelParams, SECTION_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libInstanceStixels.so")
_LIB = None

EXPORTS = [
    "ish_last_error", "ish_create", "ish_destroy", "ish_set_config", "ish_initialize",
    "ish_precompute_host",
    "ish_finish", "ish_is_initialized", "ish_real_cols", "ish_max_sections",
    "ish_get_parameters", "ish_get_luts", "ish_core_context", "ish_set_disparity_image",
    "ish_set_segmentation", "ish_set_road_parameters", "ish_get_ground_model", "ish_compute",
    "ish_get_instance_stixels", "ish_get_3d_vertices", "ish_save_stixels", "ish_time_compute",
    "ish_set_device", "ish_compute_batch", "ish_time_compute_batch", "ish_compute_batch_gather",
    "ire_create", "ire_destroy", "ire_initialize", "ire_finish", "ire_compute", "ire_get_binary",
    "ire_hough_lines", "ire_choose_line", "ire_set_device", "ire_active_device", "ire_compute_device",
    "ish_get_input_disparity_on_device", "ire_compute_batch", "ire_set_batch_limits", "ire_batch_fallbacks",
    "ish_render_batch",
    "ish_instance_overlap_batch", "ish_instance_overlap_records", "ish_set_instance_overlap_capacity",
    "ish_world_batch", "ish_world_records", "ish_set_world_capacity",
    "ish_instance_objects_batch", "ish_instance_objects_records", "ish_set_instance_object_capacity",
    "ish_assign_instances_gt_batch", "ish_assign_instances_gt_quads", "ish_use_cluster_instances", "ish_set_gt_assignment_parameters",
    "ish_ground_truth_offsets_batch",
    "ish_core_sweep_set", "ish_sweep_batch", "ish_select_sweep_set", "ish_last_frames", "ish_sweep_sets",
    "ish_active_device", "ish_sweep_sections", "ish_recluster_batch",
    "ish_cluster_instance_disparity_batch", "ish_set_instance_disparity_capacity",
    "ish_set_segmentation_head", "ish_set_segmentation_head_clamp", "ish_segmentation_head_batch",
    "ish_cnn_label_batch",
]
WORLD_DTYPE = _core.WORLD_DTYPE  # is_world_stixel, the records of Stixels.WorldBatch
OBJECT_DTYPE = _core.OBJECT_DTYPE    # is_instance_object, the objects of Stixels.InstanceObjectsBatch
CONTOUR_DTYPE = _core.CONTOUR_DTYPE  # is_contour_point, its contour points

# Stixels::RoadParameters, what RoadEstimation::ComputeBatch writes per frame
ROAD_PARAMETERS_DTYPE = np.dtype([("vhor", np.int32), ("camera_tilt", np.float32),
                                  ("camera_height", np.float32), ("alpha_ground", np.float32)])


class _IshConfig(ctypes.Structure):
    _f, _i = ctypes.c_float, ctypes.c_int
    _fields_ = [
        ("rows", _f), ("cols", _f), ("max_dis", _i), ("invalid_disparity", _f), ("eps", _f),
        ("min_pts", _i), ("size_filter", _i), ("n_semantic_classes", _i),
        ("n_offset_channels", _i), ("prior_weight", _f), ("segmentation_weight", _f),
        ("instance_weight", _f), ("disparity_weight", _f), ("pairwise", _i), ("column_step", _i),
        ("focal", _f), ("baseline", _f), ("camera_center_x", _f), ("camera_center_y", _f),
        ("sigma_disparity_object", _f), ("sigma_disparity_ground", _f), ("sigma_sky", _f),
        ("pout", _f), ("pout_sky", _f), ("pord", _f), ("pgrav", _f), ("pblg", _f),
        ("pground_given_nexist", _f), ("pobject_given_nexist", _f), ("psky_given_nexist", _f),
        ("pnexist_dis", _f), ("pground", _f), ("pobject", _f), ("psky", _f), ("width_margin", _i),
        ("sigma_camera_tilt", _f), ("sigma_camera_height", _f), ("median_join", _i),
        ("epsilon", _f), ("range_objects_z", _f), ("road_vdisparity_threshold", _f),
    ]


def lib():
    global _LIB
    if _LIB is None:
        _core.lib()  # loads torch's HIP runtime first (if any) and libis_core.so
        if not os.path.exists(LIB_PATH):
            raise _core.CoreError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.ish_last_error.restype = ctypes.c_char_p
        L.ish_create.restype = vp
        L.ish_destroy.argtypes = [vp]
        L.ish_set_config.argtypes = [vp, ctypes.POINTER(_IshConfig)]
        L.ish_initialize.argtypes = [vp, ci]
        L.ish_finish.argtypes = [vp]
        L.ish_precompute_host.argtypes = [vp]
        L.ish_is_initialized.argtypes = [vp]
        L.ish_real_cols.argtypes = [vp]
        L.ish_max_sections.argtypes = [vp]
        L.ish_get_parameters.argtypes = [vp, ctypes.POINTER(StixelParams)]
        L.ish_get_luts.argtypes = [vp, vp, vp]
        L.ish_core_context.argtypes = [vp]
        L.ish_core_context.restype = vp
        L.ish_set_disparity_image.argtypes = [vp, vp, ctypes.c_size_t]
        L.ish_set_segmentation.argtypes = [vp, vp, ctypes.c_size_t]
        L.ish_set_road_parameters.argtypes = [vp, ci, cf, cf, cf]
        L.ish_get_ground_model.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ci)]
        L.ish_compute.argtypes = [vp, ci, vp, vp, ctypes.POINTER(cf), ctypes.POINTER(cf)]
        L.ish_get_instance_stixels.argtypes = [vp, vp, ci]
        L.ish_time_compute.argtypes = [vp, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
        L.ish_set_device.argtypes = [vp, ci]
        L.ish_compute_batch.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp]
        L.ish_compute_batch_gather.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp]
        L.ish_time_compute_batch.argtypes = [vp, ci, ci, vp, vp, vp, ci, ci,
                                             ctypes.POINTER(ctypes.c_double)]
        L.ish_get_3d_vertices.argtypes = [vp, vp, cf, ci, vp, ci]
        L.ish_save_stixels.argtypes = [vp, vp, vp, ci, cf, ci, ctypes.c_char_p]
        L.ire_create.restype = vp
        L.ire_destroy.argtypes = [vp]
        L.ire_initialize.argtypes = [vp, cf, cf, cf, ci, ci, ci, cf]
        L.ire_finish.argtypes = [vp]
        L.ire_compute.argtypes = [vp, vp, ctypes.c_size_t, vp]
        L.ire_get_binary.argtypes = [vp, vp, ctypes.c_size_t]
        L.ire_hough_lines.argtypes = [vp, ci, ci, cf, cf, ci, vp, ci]
        L.ire_choose_line.argtypes = [cf, cf, cf, ci, vp, ci, vp]
        L.ire_set_device.argtypes = [vp, ci]
        L.ire_active_device.argtypes = [vp]
        L.ire_compute_device.argtypes = [vp, vp, vp]
        L.ish_get_input_disparity_on_device.argtypes = [vp]
        L.ire_compute_batch.argtypes = [vp, vp, ci, vp, vp, vp]
        L.ire_set_batch_limits.argtypes = [vp, ci, ci]
        L.ire_batch_fallbacks.argtypes = [vp]
        L.ish_render_batch.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
        L.ish_instance_overlap_batch.argtypes = [vp, ci, vp, vp, vp]
        L.ish_instance_overlap_records.argtypes = [vp, vp, ctypes.c_int64]
        L.ish_set_instance_overlap_capacity.argtypes = [vp, ci]
        L.ish_world_batch.argtypes = [vp, ci, vp, vp]
        L.ish_world_records.argtypes = [vp, vp, ctypes.c_int64]
        L.ish_set_world_capacity.argtypes = [vp, ci]
        L.ish_instance_objects_batch.argtypes = [vp, ci, vp, vp, vp, vp]
        L.ish_instance_objects_records.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64]
        L.ish_set_instance_object_capacity.argtypes = [vp, ci]
        L.ish_get_input_disparity_on_device.restype = vp
        L.ish_assign_instances_gt_batch.argtypes = [vp, ci, vp, ctypes.POINTER(ctypes.c_int64), vp]
        L.ish_assign_instances_gt_quads.argtypes = [vp, vp, ctypes.c_int64]
        L.ish_use_cluster_instances.argtypes = [vp]
        L.ish_ground_truth_offsets_batch.argtypes = [vp, ci, vp, vp, vp]
        L.ish_set_gt_assignment_parameters.argtypes = [vp, ctypes.c_double, vp, ci]
        L.ish_set_segmentation_head.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ci]
        L.ish_set_segmentation_head_clamp.argtypes = [vp, ci, cf, cf]
        L.ish_segmentation_head_batch.argtypes = [vp, ci, vp, ci, vp, vp, vp]
        L.ish_cnn_label_batch.argtypes = [vp, ci, vp, ci, vp, vp, vp, ci, vp, vp]
        L.ish_core_sweep_set.argtypes = [vp, ctypes.POINTER(_core.SweepSet)]
        L.ish_sweep_batch.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, ci, vp]
        L.ish_select_sweep_set.argtypes = [vp, ci]
        L.ish_last_frames.argtypes = [vp]
        L.ish_sweep_sets.argtypes = [vp]
        L.ish_active_device.argtypes = [vp]
        L.ish_sweep_sections.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp]
        L.ish_recluster_batch.argtypes = [vp, cf, ci, ci, ci, vp, ci, vp, vp]
        L.ish_cluster_instance_disparity_batch.argtypes = [vp, ci, vp, vp, ci, cf, ci, ci, vp, ci, vp, vp, vp]
        L.ish_set_instance_disparity_capacity.argtypes = [vp, ci]
        for f in (L.ish_erff, L.ish_atanf, L.ish_cosf):
            f.argtypes, f.restype = [cf], cf
        for f in (L.ish_erff_n, L.ish_atanf_n, L.ish_cosf_n):
            f.argtypes, f.restype = [vp, vp, ctypes.c_size_t], None
        L.ish_precompute_ground_shared.argtypes = [vp, ci, cf, cf, cf, vp, vp, vp, vp]
        L.ish_ground_params.argtypes = [vp, ctypes.POINTER(_core.GroundParams)]
        L.ish_log_lut.argtypes = [vp, vp, ci]
        L.ish_compute_batch_road.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
        L.ire_compute_batch_device.argtypes = [vp, vp, ci, vp, vp, vp, vp]
        L.ire_choose_line_shared.argtypes = [cf, cf, cf, ci, vp, ci, ci, ci, vp, vp, ctypes.POINTER(ci)]
        L.ire_pitch_gate.argtypes, L.ire_pitch_gate.restype = [ctypes.POINTER(cf), ctypes.POINTER(cf)], None
        _LIB = L
    return _LIB


@dataclasses.dataclass
class StixelsData:               # types.h:196-205
    sections: np.ndarray         # [realcols][max_sections] SECTION_DTYPE
    rows: int
    cols: int
    realcols: int
    max_sections: int
    max_dis: int
    column_step: int
    semantic_classes: int
    alpha_ground: float
    vhor: int


class Stixels:
    def __init__(self):
        self._h = ctypes.c_void_p(lib().ish_create())
        self._cfg = None

    def _check(self, rc, what):
        if rc == -1:
            raise ValueError(lib().ish_last_error().decode())   # std::invalid_argument
        if rc < 0:
            raise RuntimeError(f"{what}: {lib().ish_last_error().decode()}")
        return rc

    def close(self):
        if self._h:
            lib().ish_finish(self._h)
            lib().ish_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API ---------------------------------------------------------------
    def SetConfig(self, cfg: StixelConfig):
        c = _IshConfig()
        for name, _ in _IshConfig._fields_:
            v = getattr(cfg, name)
            setattr(c, name, int(v) if isinstance(v, (bool, np.bool_)) else v)
        self._check(lib().ish_set_config(self._h, ctypes.byref(c)), "SetConfig")
        self._cfg = cfg

    def Initialize(self, max_batch=1):
        self._check(lib().ish_initialize(self._h, int(max_batch)), "Initialize")

    def SetDevice(self, device):
        """GPU of the next Initialize() (default: the caller's current HIP device)."""
        self._check(lib().ish_set_device(self._h, int(device)), "SetDevice")

    def GetInputDisparityImageOnDevice(self):
        """Device address of the internal full-resolution disparity buffer (Stixels.cu:357-359)."""
        return int(lib().ish_get_input_disparity_on_device(self._h) or 0)

    def time_compute(self, pairwise, n_iter=100, with_instances=False):
        """Seconds per frame of n_iter Stixels::Compute() calls timed inside the C++ library."""
        t = ctypes.c_double()
        self._check(lib().ish_time_compute(self._h, int(bool(pairwise)), int(n_iter),
                                           int(bool(with_instances)), ctypes.byref(t)),
                    "time_compute")
        return t.value

    def PrecomputeHost(self):
        """Host half of Initialize (tables + StixelParameters); needs no GPU."""
        self._check(lib().ish_precompute_host(self._h), "PrecomputeHost")

    def Finish(self):
        self._check(lib().ish_finish(self._h), "Finish")

    def IsInitialized(self):
        return bool(lib().ish_is_initialized(self._h))

    def GetRealCols(self):
        return lib().ish_real_cols(self._h)

    def GetMaxSections(self):
        return lib().ish_max_sections(self._h)

    def SetDisparityImage(self, disp):
        a = np.ascontiguousarray(disp, np.float32)
        self._check(lib().ish_set_disparity_image(self._h, a.ctypes.data, a.size),
                    "SetDisparityImage")

    def SetSegmentation(self, seg):
        a = np.ascontiguousarray(seg, np.int32)
        self._check(lib().ish_set_segmentation(self._h, a.ctypes.data, a.size), "SetSegmentation")

    def SetRoadParameters(self, vhor, camera_tilt, camera_height, alpha_ground):
        self._check(lib().ish_set_road_parameters(self._h, int(vhor), camera_tilt, camera_height,
                                                  alpha_ground), "SetRoadParameters")

    def Compute(self, pairwise) -> StixelsData:
        C, S = self.GetRealCols(), self.GetMaxSections()
        sec = np.zeros((C, S), SECTION_DTYPE)
        hdr = np.zeros(9, np.int32)
        alpha, ret = ctypes.c_float(), ctypes.c_float()
        self._check(lib().ish_compute(self._h, int(bool(pairwise)), sec.ctypes.data,
                                      hdr.ctypes.data, ctypes.byref(alpha), ctypes.byref(ret)),
                    "Compute")
        return StixelsData(sec, *[int(x) for x in hdr[:7]], float(alpha.value), int(hdr[7]))

    def ComputeBatch(self, pairwise, d_disparity_big, d_segmentation, road, with_instances=True,
                     stream=0):
        """Stixels::ComputeBatch on device-resident inputs (device pointers as ints):
        d_disparity_big [n][rows][cols] f32, d_segmentation [n][realcols][channels][P2S] i32,
        road: n tuples (vhor_image, camera_tilt, camera_height, alpha_ground).
        Returns (list of StixelsData, list of instance mappings or None)."""
        n = len(road)
        C, S = self.GetRealCols(), self.GetMaxSections()
        rp = np.ascontiguousarray(road, np.float32).reshape(n, 4)
        sec = np.zeros((n, C, S), SECTION_DTYPE)
        vh = np.zeros(n, np.int32)
        cap = C * S
        tri = np.zeros((n, cap, 3), np.int32) if with_instances else None
        cnt = np.zeros(n, np.int32)
        self._check(lib().ish_compute_batch(self._h, int(bool(pairwise)), n, d_disparity_big,
                                            d_segmentation, rp.ctypes.data, sec.ctypes.data,
                                            vh.ctypes.data, tri.ctypes.data if with_instances else None,
                                            cap, cnt.ctypes.data, stream), "ComputeBatch")
        cfg = self._cfg
        data = [StixelsData(sec[i], int(cfg.rows), int(cfg.cols), C, S, int(cfg.max_dis),
                            int(cfg.column_step), int(cfg.n_semantic_classes), float(rp[i, 3]),
                            int(vh[i])) for i in range(n)]
        maps = None
        if with_instances:
            maps = [{(int(u), int(v)): int(l) for u, v, l in tri[i, :cnt[i]]} for i in range(n)]
        return data, maps

    def ComputeBatchRoad(self, pairwise, n, d_disparity_big, d_segmentation, d_road, d_status, with_instances=True,
                         stream=0):
        """Stixels::ComputeBatchRoad: ComputeBatch with the road records d_road [n] (16 bytes each) and the status
        bytes d_status [n] on the device (RoadEstimation.ComputeBatchDevice); the ground model is built on the
        device.  Returns (list of StixelsData, mappings or None, road, status): road n tuples (vhor_image,
        camera_tilt, camera_height, alpha_ground) and status n ints (core.ROAD_*), from the copy the call fetched
        behind the DP."""
        C, S = self.GetRealCols(), self.GetMaxSections()
        sec = np.zeros((n, C, S), SECTION_DTYPE)
        vh = np.zeros(n, np.int32)
        alpha = np.zeros(n, np.float32)
        rp = np.zeros((n, 4), np.float32)
        st = np.zeros(n, np.uint8)
        cap = C * S
        tri = np.zeros((n, cap, 3), np.int32) if with_instances else None
        cnt = np.zeros(n, np.int32)
        self._check(lib().ish_compute_batch_road(self._h, int(bool(pairwise)), int(n), d_disparity_big, d_segmentation,
                                                 d_road, d_status, sec.ctypes.data, vh.ctypes.data, alpha.ctypes.data,
                                                 rp.ctypes.data, st.ctypes.data,
                                                 tri.ctypes.data if with_instances else None, cap, cnt.ctypes.data,
                                                 stream), "ComputeBatchRoad")
        cfg = self._cfg
        data = [StixelsData(sec[i], int(cfg.rows), int(cfg.cols), C, S, int(cfg.max_dis), int(cfg.column_step),
                            int(cfg.n_semantic_classes), float(alpha[i]), int(vh[i])) for i in range(n)]
        maps = _maps(tri, cnt) if with_instances else None
        road = [(int(r[0]), np.float32(r[1]), np.float32(r[2]), np.float32(r[3])) for r in rp]
        return data, maps, road, [int(x) for x in st]

    def PrecomputeGroundShared(self, vhor_lib, camera_tilt, camera_height, alpha_ground):
        """Stixels::PrecomputeGroundShared with this object's constants (after PrecomputeHost() or Initialize()): the
        host twin of the device ground model.  Returns (function, normalization, inv_sigma2, range_index), [rows]
        each; range_index is the FastLog index of the a_range term."""
        H = self.GetParameters().rows
        gf, ng, ig = (np.zeros(H, np.float32) for _ in range(3))
        idx = np.zeros(H, np.int32)
        self._check(lib().ish_precompute_ground_shared(self._h, int(vhor_lib), camera_tilt, camera_height,
                                                       alpha_ground, gf.ctypes.data, ng.ctypes.data, ig.ctypes.data,
                                                       idx.ctypes.data), "PrecomputeGroundShared")
        return gf, ng, ig, idx

    def GroundParams(self):
        """core.GroundParams of this object's configuration (Core.set_ground_model)."""
        gp = _core.GroundParams()
        self._check(lib().ish_ground_params(self._h, ctypes.byref(gp)), "GroundParams")
        return gp

    def GetLogLUT(self):
        """The table Stixels::FastLog reads (after PrecomputeHost() or Initialize())."""
        n = int(lib().ish_log_lut(self._h, None, 0))
        out = np.zeros(n, np.float32)
        lib().ish_log_lut(self._h, out.ctypes.data, n)
        return out

    def ComputeBatchGather(self, pairwise, d_disparity_big, d_segmentation, road, comm, dst,
                           images_per_rank, road_all=None, stream=0):
        """Stixels::ComputeBatchGather: this rank's shard, then the RCCL gather of every rank's Sections on
        rank `dst` of `comm` (an ncclComm_t as int, core.comm_init_rank).  road: this rank's tuples
        (vhor_image, camera_tilt, camera_height, alpha_ground); road_all: those of ALL frames in rank
        order (dst only).  Returns the list of StixelsData of all frames on dst, [] elsewhere."""
        n = len(road)
        C, S = self.GetRealCols(), self.GetMaxSections()
        rp = np.ascontiguousarray(road, np.float32).reshape(n, 4)
        ipr = np.ascontiguousarray(images_per_rank, np.int32)
        n_all = int(ipr.sum())
        ra = None if road_all is None else np.ascontiguousarray(road_all, np.float32).reshape(n_all, 4)
        sec = np.zeros((n_all, C, S), SECTION_DTYPE)
        vh = np.zeros(n_all, np.int32)
        n_out = ctypes.c_int(0)
        self._check(lib().ish_compute_batch_gather(
            self._h, int(bool(pairwise)), n, d_disparity_big, d_segmentation, rp.ctypes.data,
            ctypes.c_void_p(int(comm)), int(dst), ipr.ctypes.data, None if ra is None else ra.ctypes.data, n_all,
            sec.ctypes.data, vh.ctypes.data, ctypes.byref(n_out), stream), "ComputeBatchGather")
        cfg = self._cfg
        return [StixelsData(sec[i], int(cfg.rows), int(cfg.cols), C, S, int(cfg.max_dis), int(cfg.column_step),
                            int(cfg.n_semantic_classes), float(ra[i, 3]), int(vh[i])) for i in range(n_out.value)]

    def time_compute_batch(self, pairwise, d_disparity_big, d_segmentation, road, n_iter=5,
                           with_instances=False):
        """Seconds per ComputeBatch() call, timed inside the C++ library."""
        rp = np.ascontiguousarray(road, np.float32).reshape(len(road), 4)
        t = ctypes.c_double()
        self._check(lib().ish_time_compute_batch(self._h, int(bool(pairwise)), len(road),
                                                 d_disparity_big, d_segmentation, rp.ctypes.data,
                                                 int(n_iter), int(bool(with_instances)),
                                                 ctypes.byref(t)), "time_compute_batch")
        return t.value

    def RenderBatch(self, n, label=None, disparity=None, instance=None, gt_label=None, n_labels=34,
                    confusion=None, gt_disparity=None, stream=0, class_to_label=None):
        """Stixels::RenderBatch: frames 0 .. n-1 of the last Compute() / ComputeBatch() to dense per-pixel maps
        and scores on the device (device pointers as ints, None = skipped; see is_render_sections):
        label [n][rows][cols] u8 labelIds, disparity f32, instance i32; gt_label u8 with confusion
        [n_labels][n_labels] u64 (added to); gt_disparity f32 for the deviation.  class_to_label: host table of
        label values per semantic class (None: Cityscapes trainId -> labelId).
        Returns (disp_abs_sum [n] f64, disp_count [n] i64, stixel_count [n] i32) as numpy arrays."""
        n = int(n)
        sums = np.zeros(max(n, 0), np.float64)
        counts = np.zeros(max(n, 0), np.int64)
        stixels = np.zeros(max(n, 0), np.int32)
        table = None if class_to_label is None else np.ascontiguousarray(class_to_label, np.uint8)
        p = lambda x: None if x is None else ctypes.c_void_p(int(x))  # noqa: E731
        self._check(lib().ish_render_batch(
            self._h, n, p(label), p(disparity), p(instance), p(gt_label), int(n_labels), p(confusion),
            p(gt_disparity), None if table is None else table.ctypes.data, 0 if table is None else table.size,
            sums.ctypes.data, counts.ctypes.data, stixels.ctypes.data, ctypes.c_void_p(int(stream))),
            "RenderBatch")
        return sums, counts, stixels

    def InstanceOverlapBatch(self, n, d_gt, stream=0):
        """Stixels::InstanceOverlapBatch: per frame 0 .. n-1 of the last Compute() / ComputeBatch(), the sparse joint
        histogram of its instance image and the ground-truth instanceIds d_gt (device int32 [n][rows][cols], an
        int pointer): a numpy array of core.OVERLAP_DTYPE (pred, gt, count), ascending by (pred, gt), summing to
        rows*cols.  Returns a list of n such arrays."""
        n = int(n)
        counts = np.zeros(max(n, 0), np.int64)
        self._check(lib().ish_instance_overlap_batch(self._h, n, ctypes.c_void_p(int(d_gt)) if d_gt else None,
                                                     counts.ctypes.data, ctypes.c_void_p(int(stream))),
                    "InstanceOverlapBatch")
        flat = np.zeros(int(counts.sum()), _core.OVERLAP_DTYPE)
        self._check(lib().ish_instance_overlap_records(self._h, flat.ctypes.data if flat.size else None,
                                                       flat.size), "InstanceOverlapBatch")
        return np.split(flat, np.cumsum(counts)[:-1]) if n > 0 else []

    def SetInstanceOverlapCapacity(self, records):
        """Records per frame of InstanceOverlapBatch's first pass (frames beyond it are repeated with more)."""
        self._check(lib().ish_set_instance_overlap_capacity(self._h, int(records)), "SetInstanceOverlapCapacity")

    def WorldBatch(self, n, stream=0, out=None):
        """Stixels::WorldBatch: the 3-D stixel world of frames 0 .. n-1 of the last Compute() / ComputeBatch(),
        built on the device: (frame_offsets [n+1] int32, records) with records a numpy array of WORLD_DTYPE
        (is_world_stixel) in (frame, column, section) order; frame f is records[frame_offsets[f]:frame_offsets[f+1]].
        The records are copied ONCE on the host, out of the object's pinned buffer.  out: a C-contiguous WORLD_DTYPE
        array the caller keeps from batch to batch; where it holds the batch, records is a view of its head and no
        memory is allocated (a fresh array of a 64-frame batch at 1024x2048 is ~89 MB of new pages per call, which
        costs more than the copy itself)."""
        n = int(n)
        offsets = np.zeros(max(n, 0) + 1, np.int32)
        self._check(lib().ish_world_batch(self._h, n, offsets.ctypes.data, ctypes.c_void_p(int(stream))),
                    "WorldBatch")
        total = int(offsets[-1])
        if out is not None and (out.dtype != WORLD_DTYPE or out.ndim != 1 or not out.flags.c_contiguous):
            raise ValueError("WorldBatch: out must be a C-contiguous 1-D array of WORLD_DTYPE")
        records = out[:total] if out is not None and out.size >= total else np.empty(total, WORLD_DTYPE)
        self._check(lib().ish_world_records(self._h, records.ctypes.data if total else None, total), "WorldBatch")
        return offsets, records

    def InstanceObjectsBatch(self, n, stream=0):
        """Stixels::InstanceObjectsBatch: the per-instance form of frames 0 .. n-1 of the last Compute() /
        ComputeBatch(), reduced on the device: (objects, points, frame_objects, frame_points) with objects a numpy
        array of OBJECT_DTYPE (is_instance_object) ascending by (frame, class, label), points one of CONTOUR_DTYPE
        (is_contour_point) ascending by (object, column) -- object o owns points[first_point : first_point +
        n_columns] -- and the objects / points of every frame as int32 [n].  The instance ids are the cluster labels,
        or the ground-truth vote after AssignInstancesGTBatch.  world.instance_objects turns the two arrays into
        boxes, mean disparities and 3-D contours."""
        n = int(n)
        frame_objects, frame_points = np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int32)
        totals = np.zeros(2, np.int32)
        self._check(lib().ish_instance_objects_batch(self._h, n, frame_objects.ctypes.data, frame_points.ctypes.data,
                                                     totals.ctypes.data, ctypes.c_void_p(int(stream))),
                    "InstanceObjectsBatch")
        objects, points = np.empty(int(totals[0]), OBJECT_DTYPE), np.empty(int(totals[1]), CONTOUR_DTYPE)
        self._check(lib().ish_instance_objects_records(self._h, objects.ctypes.data, objects.size,
                                                       points.ctypes.data, points.size), "InstanceObjectsBatch")
        return objects, points, frame_objects, frame_points

    def SetInstanceObjectCapacity(self, objects_per_frame):
        """Objects per frame InstanceObjectsBatch's first pass has room for (a batch beyond it is repeated once with
        its true totals; the object keeps the larger buffers)."""
        self._check(lib().ish_set_instance_object_capacity(self._h, int(objects_per_frame)),
                    "SetInstanceObjectCapacity")

    def AssignInstancesGTBatch(self, n, d_gt, stream=0, with_mapping=True):
        """Stixels::AssignInstancesGTBatch: the instance id of every stixel of frames 0 .. n-1 of the last Compute() /
        ComputeBatch() by majority vote over the ground-truth instanceIds d_gt (device int32 [n][rows][cols], an int
        pointer), as the reference tooling's assign_instances_gt.  From then on RenderBatch, InstanceOverlapBatch and
        WorldBatch take their instance ids from this vote, until the next compute call or UseClusterInstances().
        Returns per frame {(column, section): label} of every labelled section, or None without with_mapping."""
        n = int(n)
        p = ctypes.c_void_p(int(d_gt)) if d_gt else None
        k = ctypes.c_int64(0)
        self._check(lib().ish_assign_instances_gt_batch(self._h, n, p, ctypes.byref(k) if with_mapping else None,
                                                        ctypes.c_void_p(int(stream))), "AssignInstancesGTBatch")
        if not with_mapping:
            return None
        quads = np.empty((k.value, 4), np.int32)
        self._check(lib().ish_assign_instances_gt_quads(self._h, quads.ctypes.data if k.value else None, k.value),
                    "AssignInstancesGTBatch")
        maps = [{} for _ in range(n)]
        for f, u, v, l in quads.tolist():
            maps[f][(u, v)] = l
        return maps

    def GroundTruthOffsetsBatch(self, n, d_gt, d_segmentation, stream=0):
        """Stixels::GroundTruthOffsetsBatch: channels 19 and 20 of d_segmentation (device int32
        [n][cols / 8][21][P2S], an int pointer) from the ground-truth instanceIds d_gt (device int32 [n][rows][cols]),
        the reference's --usegtoffsets producer; the class channels are not touched.  A producer: legal before any
        compute call, asynchronous on `stream`."""
        self._check(lib().ish_ground_truth_offsets_batch(
            self._h, int(n), ctypes.c_void_p(int(d_gt)) if d_gt else None,
            ctypes.c_void_p(int(d_segmentation)) if d_segmentation else None, ctypes.c_void_p(int(stream))),
            "GroundTruthOffsetsBatch")

    # ---- the CNN's segmentation head ----------------------------------------------------
    def SetSegmentationHead(self, weight, bias, K):
        """Stixels::SetSegmentationHead: seg.weight [channels][K] and seg.bias [channels] of the head's 1x1 convolution
        (host arrays), channels = the configured classes + instance channels.  ValueError on mismatched sizes; needs
        no device."""
        w = np.ascontiguousarray(weight, np.float32).reshape(-1)
        b = np.ascontiguousarray(bias, np.float32).reshape(-1)
        self._check(lib().ish_set_segmentation_head(self._h, w.ctypes.data, w.size, b.ctypes.data, b.size, int(K)),
                    "SetSegmentationHead")

    def SetSegmentationHeadClamp(self, channel, lo=0.0, hi=0.0):
        """Stixels::SetSegmentationHeadClamp: one regression channel clamped to [lo, hi]; channel -1: none."""
        self._check(lib().ish_set_segmentation_head_clamp(self._h, int(channel), float(lo), float(hi)),
                    "SetSegmentationHeadClamp")

    def SegmentationHeadBatch(self, n, d_features, dtype, d_segmentation, d_cnn_out=0, stream=0):
        """Stixels::SegmentationHeadBatch (device pointers as ints): d_features [n][K][rows / 8][realcols] of dtype
        core.HEAD_F32 / HEAD_F16 / HEAD_BF16 -> d_segmentation [n][realcols][channels][P2S] int32, what ComputeBatch
        takes, and optionally d_cnn_out [n][channels][rows / 8][realcols] float32.  A producer: legal before any
        compute call, one asynchronous launch on `stream`."""
        self._check(lib().ish_segmentation_head_batch(
            self._h, int(n), ctypes.c_void_p(int(d_features)) if d_features else None, int(dtype),
            ctypes.c_void_p(int(d_segmentation)) if d_segmentation else None,
            ctypes.c_void_p(int(d_cnn_out)) if d_cnn_out else None, ctypes.c_void_p(int(stream))),
            "SegmentationHeadBatch")

    def CnnLabelBatch(self, n, d_cnn_out, mode, d_class8=0, d_label=0, d_gt_label=0, n_labels=34, d_confusion=0,
                      stream=0):
        """Stixels::CnnLabelBatch (device pointers as ints): d_cnn_out [n][channels][rows / 8][realcols] float32, the
        float output of SegmentationHeadBatch, and mode core.CNN_UP_NEAREST / CNN_UP_DECONV -> the optional d_class8
        [n][rows / 8][realcols] and d_label [n][rows][cols] uint8, and with d_gt_label [n][rows][cols] uint8 the
        confusion table d_confusion [n_labels][n_labels] uint64, which is added to.  A producer: legal before any
        compute call, one asynchronous launch on `stream`."""
        def p(v):
            return ctypes.c_void_p(int(v)) if v else None
        self._check(lib().ish_cnn_label_batch(self._h, int(n), p(d_cnn_out), int(mode), p(d_class8), p(d_label),
                                              p(d_gt_label), int(n_labels), p(d_confusion), p(stream)),
                    "CnnLabelBatch")

    # ---- parameter sweeps ------------------------------------------------------------
    def SweepBatch(self, pairwise, d_disparity_big, d_segmentation, road, sets, with_instances=True, stream=0):
        """Stixels::SweepBatch: ComputeBatch for every parameter set of `sets` on the same device-resident inputs in
        one call.  sets: tuples (prior_weight, disparity_weight, segmentation_weight, instance_weight, eps, min_pts,
        size_filter), the weights as SetWeightParameters takes them.  The results stay on the device; set 0 is
        selected for the consumers (RenderBatch, InstanceOverlapBatch, WorldBatch, AssignInstancesGTBatch,
        InstanceObjectsBatch), SelectSweepSet chooses another, SweepSections brings one to the host."""
        n = len(road)
        rp = np.ascontiguousarray(road, np.float32).reshape(n, 4)
        ss = np.ascontiguousarray(sets, np.float32).reshape(len(sets), 7)
        self._check(lib().ish_sweep_batch(self._h, int(bool(pairwise)), n, d_disparity_big, d_segmentation,
                                          rp.ctypes.data, ss.ctypes.data, len(ss), int(bool(with_instances)),
                                          stream), "SweepBatch")

    def SelectSweepSet(self, k):
        """Makes set k of the last SweepBatch what the consumers read; ValueError when k is out of range or the last
        compute call was not a sweep."""
        self._check(lib().ish_select_sweep_set(self._h, int(k)), "SelectSweepSet")

    def _query(self, f, what):
        v = int(f(self._h))
        if v < -1:
            raise ValueError(f"{what}: the object is closed")
        return v

    def LastFrames(self):
        """Frames of the last compute call the consumers can read."""
        return self._query(lib().ish_last_frames, "LastFrames")

    def SweepSets(self):
        """Sets of the last SweepBatch while it is what the consumers read; 0 when the last compute call was not a
        sweep."""
        return self._query(lib().ish_sweep_sets, "SweepSets")

    def GetActiveDevice(self):
        """The device the buffers of the last Initialize() live on (-1 before)."""
        return self._query(lib().ish_active_device, "GetActiveDevice")

    def SweepSections(self, k, with_instances=True):
        """Stixels::SweepSections: set k of the last SweepBatch on the host, as ComputeBatch returns a batch:
        (list of StixelsData, list of instance mappings or None)."""
        n = self.LastFrames()
        C, S = self.GetRealCols(), self.GetMaxSections()
        sec = np.zeros((n, C, S), SECTION_DTYPE)
        vh = np.zeros(n, np.int32)
        alpha = np.zeros(n, np.float32)
        cap = C * S
        tri = np.zeros((n, cap, 3), np.int32) if with_instances else None
        cnt = np.zeros(n, np.int32)
        self._check(lib().ish_sweep_sections(self._h, int(k), sec.ctypes.data, vh.ctypes.data, alpha.ctypes.data,
                                             tri.ctypes.data if with_instances else None, cap, cnt.ctypes.data),
                    "SweepSections")
        cfg = self._cfg
        data = [StixelsData(sec[i], int(cfg.rows), int(cfg.cols), C, S, int(cfg.max_dis), int(cfg.column_step),
                            int(cfg.n_semantic_classes), float(alpha[i]), int(vh[i])) for i in range(n)]
        return data, (_maps(tri, cnt) if with_instances else None)

    def ReclusterBatch(self, eps, min_pts, size_filter, with_mapping=True, stream=0):
        """Stixels::ReclusterBatch: the clustering of the last compute call (or of the selected sweep set) again with
        these parameters, without its DP.  Returns the per-frame instance mappings, or None without with_mapping.
        ValueError before any compute call and after one without instances."""
        n = self.LastFrames()
        cap = self.GetRealCols() * self.GetMaxSections()
        tri = np.zeros((n, cap, 3), np.int32) if with_mapping else None
        cnt = np.zeros(max(n, 1), np.int32)
        self._check(lib().ish_recluster_batch(self._h, float(eps), int(min_pts), int(size_filter), n,
                                              tri.ctypes.data if with_mapping else None, cap, cnt.ctypes.data,
                                              stream), "ReclusterBatch")
        return _maps(tri, cnt[:n]) if with_mapping else None

    def ClusterInstanceDisparityBatch(self, n, gt_instance, disparity_u8, eps, min_pts, size_filter, with_mapping=True,
                                      with_stixel_median=False, stream=0):
        """Stixels::ClusterInstanceDisparityBatch: the instance ids of frames 0 .. n-1 of the last compute call (or of
        the selected sweep set) by DBSCAN over (instance_mean_x, instance_mean_y, instance disparity), the reference
        tooling's --use-disparity from_gt.  gt_instance (int32 [n][rows][cols], Cityscapes instanceIds) and
        disparity_u8 (uint8 [n][rows][cols]) are both numpy arrays, copied to the device by the call, or both device
        pointers (ints) of resident arrays.  The labels are rewritten as ReclusterBatch rewrites them.  Returns
        (mappings or None, stixel medians float32 [n][realcols][max_sections] or None).  ValueError before any compute
        call and after one without instances; RuntimeError, with every label unchanged, when a frame holds more
        ground-truth instances than SetInstanceDisparityCapacity allows."""
        n = int(n)
        on_host = isinstance(gt_instance, np.ndarray)
        if on_host != isinstance(disparity_u8, np.ndarray):
            raise ValueError("ClusterInstanceDisparityBatch: gt_instance and disparity_u8 must both be numpy arrays "
                             "or both be device pointers")
        if on_host:
            px = max(n, 0) * int(self._cfg.rows) * int(self._cfg.cols)
            gt_instance = np.ascontiguousarray(gt_instance, np.int32)
            disparity_u8 = np.ascontiguousarray(disparity_u8, np.uint8)
            if gt_instance.size < px or disparity_u8.size < px:
                raise ValueError("ClusterInstanceDisparityBatch: an image array holds fewer than n frames")
            gt_p, disp_p = gt_instance.ctypes.data, disparity_u8.ctypes.data
        else:
            gt_p = ctypes.c_void_p(int(gt_instance)) if gt_instance else None
            disp_p = ctypes.c_void_p(int(disparity_u8)) if disparity_u8 else None
        C, S = self.GetRealCols(), self.GetMaxSections()
        cap = C * S
        tri = np.zeros((max(n, 0), cap, 3), np.int32) if with_mapping else None
        cnt = np.zeros(max(n, 1), np.int32)
        med = np.zeros((max(n, 0), C, S), np.float32) if with_stixel_median else None
        self._check(lib().ish_cluster_instance_disparity_batch(
            self._h, n, gt_p, disp_p, int(on_host), float(eps), int(min_pts), int(size_filter),
            tri.ctypes.data if with_mapping else None, cap, cnt.ctypes.data,
            med.ctypes.data if with_stixel_median else None, ctypes.c_void_p(int(stream))),
            "ClusterInstanceDisparityBatch")
        return (_maps(tri, cnt[:n]) if with_mapping else None), med

    def SetInstanceDisparityCapacity(self, keys_per_frame):
        """Ground-truth instances per frame ClusterInstanceDisparityBatch has histogram slots for (default 256)."""
        self._check(lib().ish_set_instance_disparity_capacity(self._h, int(keys_per_frame)),
                    "SetInstanceDisparityCapacity")

    def UseClusterInstances(self):
        """Back to the cluster labels of the last compute call for RenderBatch / InstanceOverlapBatch / WorldBatch."""
        self._check(lib().ish_use_cluster_instances(self._h), "UseClusterInstances")

    def SetGTAssignmentParameters(self, min_fraction=0.1, label_ids=None, gt_is_train_ids=False):
        """The parameters of AssignInstancesGTBatch: the minimum fraction of the reference's 10 % rule, the labelIds of
        classes 11..18 (None: Cityscapes 24, 25, 26, 27, 28, 31, 32, 33), and whether the ground truth is in trainId
        form (class*1000 + k)."""
        ids = None if label_ids is None else np.ascontiguousarray(label_ids, np.int32)
        if ids is not None and ids.size != 8:
            raise ValueError("SetGTAssignmentParameters: label_ids must hold 8 ids")
        self._check(lib().ish_set_gt_assignment_parameters(self._h, float(min_fraction),
                                                           None if ids is None else ids.ctypes.data,
                                                           int(bool(gt_is_train_ids))), "SetGTAssignmentParameters")

    def SetWorldCapacity(self, records_per_frame):
        """Records per frame of WorldBatch's first pass (a batch beyond it is repeated with its true total);
        0: back to the default, the exact size after a ComputeBatch and 4096 per frame after a Compute()."""
        self._check(lib().ish_set_world_capacity(self._h, int(records_per_frame)), "SetWorldCapacity")

    def GetInstanceStixels(self):
        cap = self.GetRealCols() * self.GetMaxSections()
        t = np.zeros((cap, 3), np.int32)
        n = self._check(lib().ish_get_instance_stixels(self._h, t.ctypes.data, cap),
                        "GetInstanceStixels")
        return {(int(u), int(v)): int(l) for u, v, l in t[:n]}

    def Get3DVertices(self, data: StixelsData):
        cap = data.sections.size * 12
        out = np.zeros(cap, np.float32)
        sec = np.ascontiguousarray(data.sections)
        n = self._check(lib().ish_get_3d_vertices(self._h, sec.ctypes.data, data.alpha_ground,
                                                  data.vhor, out.ctypes.data, cap),
                        "Get3DVertices")
        return out[:n].copy()

    def SaveStixels(self, data: StixelsData, instance_stixels, alpha_ground, vhor, fname):
        t = np.array([[u, v, l] for (u, v), l in instance_stixels.items()],
                     np.int32).reshape(-1, 3)
        sec = np.ascontiguousarray(data.sections)
        self._check(lib().ish_save_stixels(self._h, sec.ctypes.data, t.ctypes.data, len(t),
                                           alpha_ground, int(vhor), fname.encode()),
                    "SaveStixels")

    # ---- introspection ---------------------------------------------------------------
    def GetParameters(self) -> StixelParams:
        p = StixelParams()
        lib().ish_get_parameters(self._h, ctypes.byref(p))
        return p

    def GetLUTs(self):
        D = self.GetParameters().max_dis
        lut = np.zeros((D, D), np.float32)
        odr = np.zeros(D, np.float32)
        lib().ish_get_luts(self._h, lut.ctypes.data, odr.ctypes.data)
        return lut, odr

    def GetGroundModel(self):
        H = self.GetParameters().rows
        gf, ng, ig = (np.zeros(H, np.float32) for _ in range(3))
        vh = ctypes.c_int()
        self._check(lib().ish_get_ground_model(self._h, gf.ctypes.data, ng.ctypes.data,
                                               ig.ctypes.data, ctypes.byref(vh)),
                    "GetGroundModel")
        return gf, ng, ig, vh.value


def _maps(tri, cnt):
    """[frames][cap][3] (column, section, label) triples and their counts as one dict per frame"""
    return [{(int(u), int(v)): int(l) for u, v, l in tri[i, :cnt[i]]} for i in range(len(cnt))]


def core_sweep_set(prior_weight, disparity_weight, segmentation_weight, instance_weight, eps, min_pts, size_filter):
    """Stixels::CoreSweepSet: a SweepBatch set as the core takes it (core.SweepSet): SetWeightParameters' rule for the
    instance weight.  Needs no device."""
    s = np.array([prior_weight, disparity_weight, segmentation_weight, instance_weight, eps, min_pts, size_filter],
                 np.float32)
    out = _core.SweepSet()
    if lib().ish_core_sweep_set(s.ctypes.data, ctypes.byref(out)) < 0:
        raise RuntimeError(lib().ish_last_error().decode())
    return out


def hough_lines(image, rho=1.0, theta=float(np.pi / 180), threshold=25, cap=4096):
    """Standard Hough transform of the host library (RoadEstimation::HoughLines)."""
    img = np.ascontiguousarray(image, np.uint8)
    out = np.zeros((cap, 2), np.float32)
    n = lib().ire_hough_lines(img.ctypes.data, img.shape[0], img.shape[1], rho, theta, threshold,
                              out.ctypes.data, cap)
    return out[:min(n, cap)].copy()


def choose_line(lines, camera_center_y, baseline, focal, rows):
    """RoadEstimation::ChooseLine on lines [n][2] (rho, theta), for a camera and a v-disparity image of `rows`
    rows; needs no device.  Returns (index, road): the index of the first line whose pitch passes the gate and
    its (vhor_image, camera_tilt, camera_height, alpha_ground), or (-1, None)."""
    l = np.ascontiguousarray(lines, np.float32).reshape(-1, 2)
    out = np.zeros(1, ROAD_PARAMETERS_DTYPE)
    k = int(lib().ire_choose_line(camera_center_y, baseline, focal, int(rows), l.ctypes.data, len(l), out.ctypes.data))
    if k < 0:
        return -1, None
    r = out[0]
    return k, (int(r["vhor"]), np.float32(r["camera_tilt"]), np.float32(r["camera_height"]), np.float32(r["alpha_ground"]))


def _shared(fn, x):
    a = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(a)
    fn(a.ctypes.data, out.ctypes.data, a.size)
    return out


def is_erff(x):
    """is_erff of is_numerics.h, elementwise (float32 in, float32 out): the erf host and device share."""
    return _shared(lib().ish_erff_n, x)


def is_atanf(x):
    return _shared(lib().ish_atanf_n, x)


def is_cosf(x):
    return _shared(lib().ish_cosf_n, x)


def pitch_gate():
    """(min_pitch, max_pitch) of RoadEstimation::Initialize, as float32"""
    lo, hi = ctypes.c_float(), ctypes.c_float()
    lib().ire_pitch_gate(ctypes.byref(lo), ctypes.byref(hi))
    return np.float32(lo.value), np.float32(hi.value)


def choose_line_shared(lines, total, overflow, max_lines, camera_center_y, baseline, focal, rows,
                       fallback=(0, 0.0, 0.0, 0.0)):
    """RoadEstimation::ChooseLineShared, the host twin of is_road_choose_batch: lines [>= min(total, max_lines)][2]
    as is_road_hough_batch leaves them.  Returns (status, index, road): core.ROAD_*, the accepted line or -1, and
    (vhor_image, camera_tilt, camera_height, alpha_ground) -- the fallback unless the status is ROAD_OK."""
    l = np.ascontiguousarray(lines, np.float32).reshape(-1, 2)
    assert len(l) >= min(int(total), int(max_lines)) or overflow
    fb = np.array(fallback, np.float32)
    out = np.zeros(1, ROAD_PARAMETERS_DTYPE)
    idx = ctypes.c_int(-1)
    st = int(lib().ire_choose_line_shared(camera_center_y, baseline, focal, int(rows), l.ctypes.data, int(total),
                                          int(overflow), int(max_lines), fb.ctypes.data, out.ctypes.data,
                                          ctypes.byref(idx)))
    r = out[0]
    return st, int(idx.value), (int(r["vhor"]), np.float32(r["camera_tilt"]), np.float32(r["camera_height"]),
                                np.float32(r["alpha_ground"]))


class RoadEstimation:
    """Python view of the C++ RoadEstimation class (RoadEstimation.h of the reference)."""

    def __init__(self):
        self._h = ctypes.c_void_p(lib().ire_create())
        self._shape = None

    def Initialize(self, camera_center_y, baseline, focal, rows, cols, max_dis,
                   road_vdisparity_threshold=0.2):
        rc = lib().ire_initialize(self._h, camera_center_y, baseline, focal, rows, cols, max_dis,
                                  road_vdisparity_threshold)
        if rc < 0:
            raise RuntimeError(lib().ish_last_error().decode())
        self._shape = (rows, max_dis)

    def Compute(self, disparity):
        a = np.ascontiguousarray(disparity, np.float32)
        out = np.zeros(4, np.float32)
        rc = lib().ire_compute(self._h, a.ctypes.data, a.size, out.ctypes.data)
        if rc < 0:
            raise RuntimeError(lib().ish_last_error().decode())
        self.pitch, self.camera_height, self.slope = float(out[0]), float(out[1]), float(out[2])
        self.horizon_point = int(out[3])
        return bool(rc)

    def SetDevice(self, device):
        """Device of the next Initialize() (RoadEstimation::SetDevice, an addition like Stixels::SetDevice)."""
        lib().ire_set_device(self._h, int(device))

    def GetActiveDevice(self):
        return int(lib().ire_active_device(self._h))

    def ComputeOnDevice(self, d_ptr):
        """RoadEstimation::Compute(pixel_t* d_im): the image is on the object's device already."""
        out = np.zeros(4, np.float32)
        rc = lib().ire_compute_device(self._h, ctypes.c_void_p(int(d_ptr)), out.ctypes.data)
        if rc < 0:
            raise RuntimeError(lib().ish_last_error().decode())
        self.pitch, self.camera_height, self.slope = float(out[0]), float(out[1]), float(out[2])
        self.horizon_point = int(out[3])
        return bool(rc)

    def ComputeBatch(self, d_ptr, n, stream=0):
        """RoadEstimation::ComputeBatch on d_ptr [n][rows][cols] f32 (device pointer as int, on the object's
        device).  Returns (road, ok): road is n tuples (vhor_image, camera_tilt, camera_height, alpha_ground)
        for Stixels.ComputeBatch, ok n bools (False: no road line, the tuple is zeros)."""
        out = np.zeros(n, ROAD_PARAMETERS_DTYPE)
        ok = np.zeros(n, np.uint8)
        rc = lib().ire_compute_batch(self._h, ctypes.c_void_p(int(d_ptr)), int(n), out.ctypes.data,
                                     ok.ctypes.data, ctypes.c_void_p(int(stream)))
        if rc == -1:
            raise ValueError(lib().ish_last_error().decode())
        if rc < 0:
            raise RuntimeError(lib().ish_last_error().decode())
        road = [(int(r["vhor"]), float(r["camera_tilt"]), float(r["camera_height"]), float(r["alpha_ground"]))
                for r in out]
        return road, [bool(x) for x in ok]

    def ComputeBatchDevice(self, d_ptr, n, d_road, d_status, fallback, stream=0):
        """RoadEstimation::ComputeBatchDevice: v-disparity, Hough transform and line choice of d_ptr [n][rows][cols]
        queued on `stream`; d_road [n] 16-byte records and d_status [n] bytes (device pointers as ints) for
        Stixels.ComputeBatchRoad; fallback = (vhor_image, tilt, height, alpha).  No copy, no synchronisation."""
        fb = np.array(fallback, np.float32)
        rc = lib().ire_compute_batch_device(self._h, ctypes.c_void_p(int(d_ptr)), int(n), ctypes.c_void_p(int(d_road)),
                                            ctypes.c_void_p(int(d_status)), fb.ctypes.data,
                                            ctypes.c_void_p(int(stream)))
        if rc == -1:
            raise ValueError(lib().ish_last_error().decode())
        if rc < 0:
            raise RuntimeError(lib().ish_last_error().decode())

    def SetBatchLimits(self, max_lines, max_candidates):
        """Lines per frame and local maxima kept per frame by the device Hough transform of ComputeBatch."""
        if lib().ire_set_batch_limits(self._h, int(max_lines), int(max_candidates)) < 0:
            raise ValueError(lib().ish_last_error().decode())

    def GetBatchFallbacks(self):
        """Frames of the last ComputeBatch finished with the host Hough transform."""
        n = int(lib().ire_batch_fallbacks(self._h))
        if n < 0:
            raise ValueError("RoadEstimation is closed")
        return n

    def GetBinaryVDisparity(self):
        out = np.zeros(self._shape, np.uint8)
        lib().ire_get_binary(self._h, out.ctypes.data, out.size)
        return out

    def Finish(self):
        lib().ire_finish(self._h)

    def close(self):
        if self._h:
            lib().ire_finish(self._h)
            lib().ire_destroy(self._h)
            self._h = ctypes.c_void_p()
