"""ctypes binding of oracle/_ref/libref_stixels.so: the upstream reference's own code built for
gfx950 by `make -C oracle ref` (oracle/Makefile, oracle/ref_driver.hip).  TEST INFRASTRUCTURE ONLY.

Results come back in the layouts tests/helpers.py compares: Sections [C][S] (SECTION_DTYPE),
joined disparity [C][H], the object LUT [C][D][rows_power2 + 1], and the instance candidates as
[8][C * S](x2) arrays plus per-class counts -- in the reference's atomic arrival order, which is
unspecified; `candidate_multiset` gives an order-free view of them."""
import ctypes
import os

import numpy as np

from instance_stixels_amd.config import SECTION_DTYPE, StixelConfig

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref", "libref_stixels.so")
INSTANCE_CLASSES = 8
_LIB = None


class ReferenceError(RuntimeError):
    """The driver refused the input (outside the reference's domain) or the reference failed."""

    def __init__(self, code, message):
        super().__init__(f"reference driver error {code}: {message}")
        self.code = code


REF_E_DOMAIN = 1


def available() -> bool:
    return os.path.exists(LIB_PATH)


def lib():
    global _LIB
    if _LIB is None:
        if not available():
            raise FileNotFoundError(f"{LIB_PATH} is missing: `make -C oracle ref` with the upstream reference")
        from instance_stixels_amd import core
        core.lib()   # loads torch's HIP runtime first, as every other native library of the project
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.ref_last_error.restype = ctypes.c_char_p
        L.ref_shapes.argtypes = [vp, vp]
        L.ref_stixels_compute.argtypes = [vp, ci, vp, vp, ci, cf, cf, cf, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ref_road_vdisparity.argtypes = [vp, ci, ci, ci, cf, vp, vp, vp]
        L.ref_road_create.argtypes = [vp]
        L.ref_road_destroy.argtypes = [vp]
        L.ref_road_finish.argtypes = [vp]
        L.ref_road_initialize.argtypes = [vp, cf, cf, cf, ci, ci, ci, cf]
        L.ref_road_set_lines.argtypes = [vp, ci]
        L.ref_road_compute.argtypes = [vp, vp, ctypes.c_size_t, vp]
        L.ref_road_get.argtypes = [vp, vp, vp]
        L.ref_road_hough_call.argtypes = [vp, vp, vp, ctypes.c_size_t]
        _LIB = L
    return _LIB


def _config(cfg: StixelConfig):
    from instance_stixels_amd.host import _IshConfig   # the project's flat mirror of StixelConfig
    c = _IshConfig()
    for name, _ in _IshConfig._fields_:
        v = getattr(cfg, name)
        setattr(c, name, int(v) if isinstance(v, (bool, np.bool_)) else v)
    return c


def _check(rc):
    if rc != 0:
        raise ReferenceError(rc, lib().ref_last_error().decode(errors="replace"))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def shapes(cfg: StixelConfig):
    """(realcols, rows_power2, rows_power2_segmentation, channels) as the reference derives them;
    raises ReferenceError(REF_E_DOMAIN) for a config the driver refuses."""
    c = _config(cfg)
    out = np.zeros(4, np.int32)
    _check(lib().ref_shapes(ctypes.byref(c), _p(out)))
    return tuple(int(x) for x in out)


def stixels_compute(cfg: StixelConfig, disparity, segmentation, vhor_image, camera_tilt, camera_height,
                    alpha_ground, pairwise=None, want_lut=False):
    """One frame through the reference's Stixels class (SetConfig ... Compute ... Finish)."""
    c = _config(cfg)
    C, P2, P2S, CH = shapes(cfg)
    H, D, S = int(cfg.rows), int(cfg.max_dis), 200
    disparity = np.ascontiguousarray(disparity, np.float32)
    segmentation = np.ascontiguousarray(segmentation, np.int32)
    assert disparity.shape == (H, int(cfg.cols)), disparity.shape
    assert segmentation.shape == (C, CH, P2S), segmentation.shape
    sections = np.zeros((C, S), SECTION_DTYPE)
    joined = np.zeros((C, H), np.float32)
    lut = np.zeros((C, D, P2 + 1), np.float32) if want_lut else None
    com = np.zeros((INSTANCE_CLASSES, C * S, 2), np.float32)
    idx = np.zeros((INSTANCE_CLASSES, C * S, 2), np.int32)
    core = np.zeros((INSTANCE_CLASSES, C * S), np.uint8)
    per_class = np.zeros(INSTANCE_CLASSES, np.int32)
    vhor = ctypes.c_int(0)
    pw = cfg.pairwise if pairwise is None else pairwise
    _check(lib().ref_stixels_compute(
        ctypes.byref(c), int(bool(pw)), _p(disparity), _p(segmentation), int(vhor_image),
        ctypes.c_float(camera_tilt), ctypes.c_float(camera_height), ctypes.c_float(alpha_ground),
        _p(sections), _p(joined), _p(lut), _p(com), _p(idx), _p(core), _p(per_class), ctypes.byref(vhor)))
    return dict(sections=sections, joined=joined, object_lut=lut, inst_centerofmass=com, inst_indices=idx,
                inst_core=core, inst_per_class=per_class, vhor=vhor.value)


def stixels_compute_frame(case, image=0, want_lut=False):
    """stixels_compute on frame `image` of a tests/helpers.build_case case."""
    f = case["frames"][image]
    return stixels_compute(case["cfg"], case["disparity"][image], case["segmentation"][image], f.vhor_image,
                           f.camera_tilt, f.camera_height, f.alpha_ground, want_lut=want_lut)


def candidate_multiset(out, cls, image=None):
    """The instance candidates of one class as a sorted structured array of (col, section index,
    centre x bits, centre y bits, core flag): an order-free view (the reference appends in atomic
    arrival order, StixelsKernels.cu:927-944)."""
    def get(k):
        a = out[k]
        return a if image is None else a[image]
    n = int(get("inst_per_class")[cls])
    com = np.ascontiguousarray(get("inst_centerofmass")[cls][:n], np.float32).view(np.uint32)
    idx = get("inst_indices")[cls][:n]
    rec = np.zeros(n, [("col", np.int32), ("i", np.int32), ("x", np.uint32), ("y", np.uint32), ("core", np.uint8)])
    rec["col"], rec["i"], rec["x"], rec["y"] = idx[:, 0], idx[:, 1], com[:, 0], com[:, 1]
    rec["core"] = get("inst_core")[cls][:n] != 0
    return np.sort(rec, order=["col", "i"])


def road_vdisparity(disparity, max_dis, threshold):
    """The reference's ComputeHistogram / ComputeMaximum / ComputeBinaryImage on one frame."""
    d = np.ascontiguousarray(disparity, np.float32)
    rows, cols = d.shape
    vdisp = np.zeros((rows, max_dis), np.int32)
    binary = np.zeros((rows, max_dis), np.uint8)
    m = np.zeros(1, np.int32)
    _check(lib().ref_road_vdisparity(_p(d), rows, cols, int(max_dis), ctypes.c_float(threshold), _p(vdisp),
                                     _p(binary), _p(m)))
    return vdisp, binary, int(m[0])


class RoadEstimation:
    """The reference's RoadEstimation class.  Its cv::HoughLines is the stub of oracle/ref_stubs/opencv2:
    no transform, it returns what `set_hough_lines` installed and records its arguments (`hough_call`)."""

    def __init__(self):
        self._h = ctypes.c_void_p()
        _check(lib().ref_road_create(ctypes.byref(self._h)))

    def Initialize(self, camera_center_y, baseline, focal, rows, cols, max_dis, road_vdisparity_threshold=0.2):
        _check(lib().ref_road_initialize(self._h, camera_center_y, baseline, focal, int(rows), int(cols),
                                         int(max_dis), road_vdisparity_threshold))

    def Compute(self, disparity):
        d = np.ascontiguousarray(disparity, np.float32)
        ok = ctypes.c_int(0)
        _check(lib().ref_road_compute(self._h, _p(d), d.size, ctypes.byref(ok)))
        hp, out = ctypes.c_int(0), np.zeros(5, np.float32)
        _check(lib().ref_road_get(self._h, ctypes.byref(hp), _p(out)))
        self.horizon_point, self.pitch, self.camera_height, self.slope = hp.value, out[0], out[1], out[2]
        self.accepted_line = out[3:5].copy()       # (|rho|, theta) of the line accepted last
        return bool(ok.value)

    def Finish(self):
        _check(lib().ref_road_finish(self._h))

    def close(self):
        if self._h:
            _check(lib().ref_road_destroy(self._h))
            self._h = ctypes.c_void_p()


def set_hough_lines(lines):
    """The (rho, theta) list [n][2] the stub's cv::HoughLines returns from now on."""
    l = np.ascontiguousarray(lines, np.float32).reshape(-1, 2)
    _check(lib().ref_road_set_lines(_p(l), len(l)))


def hough_call():
    """What the stub's cv::HoughLines saw last: dict(image uint8 [rows][cols], type, rho, theta (doubles),
    threshold, calls)."""
    ints, dbl = np.zeros(5, np.int32), np.zeros(2, np.float64)
    _check(lib().ref_road_hough_call(_p(ints), _p(dbl), None, 0))
    image = np.zeros((max(int(ints[0]), 0), max(int(ints[1]), 0)), np.uint8)
    _check(lib().ref_road_hough_call(_p(ints), _p(dbl), _p(image), image.size))
    return dict(image=image, type=int(ints[2]), threshold=int(ints[3]), calls=int(ints[4]), rho=float(dbl[0]),
                theta=float(dbl[1]))
