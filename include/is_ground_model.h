/*
 * is_ground_model.h -- the per-line and per-row arithmetic of the device-resident road chain, written once for the
 * host twins (RoadEstimation::ChooseLineShared, Stixels::PrecomputeGroundShared) and for the kernels (k_road_choose,
 * k_ground_model): the same source, fp32 without contraction on both sides, and the three transcendentals taken from
 * is_numerics.h (is_erff, is_atanf, is_cosf), so that host and device give the same bits.
 *
 * Everything else is RoadEstimation::ComputeCameraProperties and Stixels::PrecomputeGround operation for operation:
 * IEEE + - * /, correctly rounded sqrtf (gcc; hipcc with -fhip-fp32-correctly-rounded-divide-sqrt), ceilf.
 * sinf / cosf of a line's theta are NOT evaluated here: theta is 0.0f + n * step for an angle index n, and the
 * caller passes the host's sinf / cosf of exactly that expression (the device reads them from a table the host
 * computed, is_road_ctx_create).
 *
 * Plain C99 / C++ / HIP.  Compile every user with -ffp-contract=off.
 */
#ifndef IS_GROUND_MODEL_H_
#define IS_GROUND_MODEL_H_

#include <math.h>

#include "instance_stixels_core.h"
#include "is_numerics.h"

/* ---- host only: the geometry of the standard Hough transform (OpenCV's HoughLinesStandard) of a width x height image,
 * stated once for RoadEstimation::HoughLines, the device transform's tables (is_road_ctx_create) and the angle index
 * of the line choice: host and device transforms agree bit for bit only while all three read it here ---- */
#define IS_ROAD_HOUGH_RHO 1.0f                                         /* the road estimation's rho ... */
#define IS_ROAD_HOUGH_THETA (3.1415926535897932384626433832795f / 180) /* ... and theta: (float)CV_PI / 180 */
static inline int is_hough_numangle(float theta) {
    const double min_theta = 0, max_theta = 3.1415926535897932384626433832795;
    return (int)lrint((max_theta - min_theta) / theta);
}
static inline int is_hough_numrho(int width, int height, float rho) {
    return (int)lrint(((width + height) * 2 + 1) / rho);
}
/* tabSin, tabCos [numangle]: the angle accumulated in fp32, its sin / cos taken in double */
static inline void is_hough_tables(int numangle, float rho, float theta, float* tabSin, float* tabCos) {
    const float irho = 1 / rho;
    float ang = 0.0f; /* (float)min_theta */
    for (int n = 0; n < numangle; ang += theta, n++) {
        tabSin[n] = (float)(sin((double)ang) * irho);
        tabCos[n] = (float)(cos((double)ang) * irho);
    }
}

/* The angle index n of a Hough line: theta == 0.0f + n * step bitwise, 0 <= n < numangle; -1 for any other theta
 * (NaN, negative, not a table angle). */
IS_HD int is_road_angle_index(float theta, float step, int numangle) {
    if (!(theta >= 0.0f) || !(theta <= (float)numangle * step)) return -1;
    const int n = (int)(theta / step + 0.5f);
    if (n < 0 || n >= numangle) return -1;
    const float back = 0.0f + n * step;
    return is_bits_f32(back) == is_bits_f32(theta) ? n : -1;
}

/* RoadEstimation::ComputeCameraProperties for a line (rho >= 0, sin and cos of its theta) and the pitch gate of
 * ComputeHough: 1 and *out = {ceil(horizon point), pitch, camera height, slope} when the pitch lies in
 * [min_pitch, max_pitch]; 0 otherwise (a NaN pitch included: theta = 0 gives rho / 0).  *vhor_ok = 0 when the
 * accepted line's horizon lies outside [0, rows): out->vhor is 0 then -- the conversion to int happens only
 * behind that range check. */
IS_HD int is_road_line(float rho, float sin_t, float cos_t, float cy, float baseline, float focal, int rows,
                       float min_pitch, float max_pitch, is_road_params* out, int* vhor_ok) {
    const float horizonPoint = rho / sin_t;
    const float pitch = -is_atanf((cy - horizonPoint) / (focal)); /* y axis is inverted */
    const float last_row = (float)(rows - 1);
    const float vDispDown = (rho - last_row * sin_t) / cos_t;
    const float slope = (0 - vDispDown) / (horizonPoint - last_row);
    const float cameraHeight = baseline * is_cosf(pitch) / slope;
    if (!(pitch >= min_pitch && pitch <= max_pitch)) return 0;
    const float top = ceilf(horizonPoint);
    *vhor_ok = top >= 0.0f && top <= last_row; /* (-0.0f: ceil of (-1, 0), row 0) */
    out->vhor = *vhor_ok ? (int)top : 0;
    out->tilt = pitch;
    out->height = cameraHeight;
    out->alpha = slope;
    return 1;
}

/* Stixels::FastLog with the index clamped to the table: [0, lut_entries - 1], a NaN reads entry 0.  Equal to the
 * host's wherever the host's index is in range (outside, the host's behaviour is undefined). */
IS_HD int is_fast_log_index(float v, int lut_entries) {
    const float f = v * (lut_entries - 1) + 0.5f;
    if (!(f >= 0.0f)) return 0;
    if (f >= (float)(lut_entries - 1)) return lut_entries - 1;
    return (int)f;
}

/* Row v of Stixels::PrecomputeGround (Stixels.cu:790-817) for the road (vhor_lib, tilt, height, alpha), with
 * is_erff in place of erff: ground_function[v], normalization_ground[v], inv_sigma2_ground[v].  *idx_range (may be
 * null) receives the FastLog index of the a_range term, for the tests' comparison with the legacy model. */
IS_HD void is_ground_row(const is_ground_params* g, const float* log_lut, int lut_entries, int vhor_lib, float tilt,
                         float height, float alpha, int v, float* fn_out, float* norm_out, float* inv_sigma2_out,
                         int* idx_range) {
    const float fb = (g->focal * g->baseline) / height;
    const float pout = g->pout;
    const float fn = alpha * (float)(vhor_lib - v); /* GroundFunction, :867-877 */
    const float x = tilt + (float)(vhor_lib - v) / g->focal;
    const float sigma2_road =
        fb * fb *
        (g->sigma_camera_height * g->sigma_camera_height * x * x / (height * height) +
         g->sigma_camera_tilt * g->sigma_camera_tilt);
    const float sigma = sqrtf(g->sigma_disparity_ground * g->sigma_disparity_ground + sigma2_road);
    const float a_range = 0.5f * (is_erff((g->max_dis - fn) / (sigma * sqrtf(2.0f))) -
                                  is_erff((-fn) / (sigma * sqrtf(2.0f))));
    const int ia = is_fast_log_index(a_range, lut_entries);
    const int ib = is_fast_log_index((1.0f - pout) / (sigma * sqrtf(2.0f * 3.1416f)), lut_entries); /* PIFLOAT */
    *fn_out = fn;
    *norm_out = log_lut[ia] - log_lut[ib];
    *inv_sigma2_out = 1.0f / (2.0f * sigma * sigma);
    if (idx_range) *idx_range = ia;
}

#endif /* IS_GROUND_MODEL_H_ */
