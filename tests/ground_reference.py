"""numpy restatement of Stixels::PrecomputeGround (Stixels.cu:790-817) in fp32, operation for operation, with the
erf left open: libm's erff gives the legacy host model, is_erff (host.is_erff) the model the device builds
(Stixels::PrecomputeGroundShared, k_ground_model).  It also returns what neither C++ function shows: the two FastLog
indices of every row, so that a test can say where the two models can differ at all.

Every numpy operation below is one IEEE fp32 operation on float32 arrays (no contraction, correctly rounded sqrt and
divide), like the C++ built with -ffp-contract=off.  tests/test_ground_device_cpu.py first pins this restatement
bitwise against both C++ functions and only then uses its indices."""
import ctypes
import ctypes.util

import numpy as np

LOG_LUT_SIZE = 1000000     # configuration.h
PIFLOAT = np.float32(3.1416)  # Stixels.hpp

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.erff.argtypes, _libm.erff.restype = [ctypes.c_float], ctypes.c_float
_libm.atanf.argtypes, _libm.atanf.restype = [ctypes.c_float], ctypes.c_float
_libm.cosf.argtypes, _libm.cosf.restype = [ctypes.c_float], ctypes.c_float


def _vec(f):
    return lambda x: np.array([f(float(v)) for v in np.asarray(x, np.float32).ravel()],
                              np.float32).reshape(np.shape(x))


libm_erff = _vec(_libm.erff)
libm_atanf = _vec(_libm.atanf)
libm_cosf = _vec(_libm.cosf)

def precompute_ground(gp, lut, rows, vhor_lib, camera_tilt, camera_height, alpha_ground, erf):
    """gp: the constants as Stixels holds them (host.Stixels.GroundParams(): focal, baseline, max_dis, pout,
    sigma_disparity_ground, sigma_camera_height, sigma_camera_tilt in radians); lut: the table FastLog reads
    (host.Stixels.GetLogLUT(), 10^6 + 1 entries).
    -> dict(function, normalization, inv_sigma2 [rows] float32; idx_range, idx_pout [rows] int64: the FastLog indices
    of the a_range term and of the (1 - pout) term, unclamped, NaN as -1; in_range [rows]: both inside the table --
    elsewhere normalization is NaN here and the C++ host path undefined)."""
    f32 = np.float32
    focal, baseline = f32(gp.focal), f32(gp.baseline)
    tilt, height, alpha = f32(camera_tilt), f32(camera_height), f32(alpha_ground)
    s_h, s_t, s_d = f32(gp.sigma_camera_height), f32(gp.sigma_camera_tilt), f32(gp.sigma_disparity_ground)
    max_dis, pout = f32(gp.max_dis), f32(gp.pout)
    with np.errstate(all="ignore"):
        fb = (focal * baseline) / height
        dv = (vhor_lib - np.arange(rows)).astype(np.float32)
        fn = alpha * dv
        x = tilt + dv / focal
        sigma2_road = fb * fb * (s_h * s_h * x * x / (height * height) + s_t * s_t)
        sigma = np.sqrt(s_d * s_d + sigma2_road)
        den = sigma * np.sqrt(f32(2.0))
        a_range = f32(0.5) * (erf((max_dis - fn) / den) - erf((-fn) / den))
        b = (f32(1.0) - pout) / (sigma * np.sqrt(f32(2.0) * PIFLOAT))
        fa = a_range * f32(LOG_LUT_SIZE) + f32(0.5)
        fb_ = b * f32(LOG_LUT_SIZE) + f32(0.5)
        ia = np.where(np.isfinite(fa), np.trunc(np.nan_to_num(fa, nan=0.0, posinf=0.0, neginf=0.0)), -1).astype(np.int64)
        ib = np.where(np.isfinite(fb_), np.trunc(np.nan_to_num(fb_, nan=0.0, posinf=0.0, neginf=0.0)), -1).astype(np.int64)
        in_range = (ia >= 0) & (ia <= LOG_LUT_SIZE) & (ib >= 0) & (ib <= LOG_LUT_SIZE)
        norm = np.full(rows, np.nan, np.float32)
        norm[in_range] = lut[ia[in_range]] - lut[ib[in_range]]
        inv_sigma2 = f32(1.0) / (f32(2.0) * sigma * sigma)
    return dict(function=fn.astype(np.float32), normalization=norm, inv_sigma2=inv_sigma2.astype(np.float32),
                idx_range=ia, idx_pout=ib, in_range=in_range)
