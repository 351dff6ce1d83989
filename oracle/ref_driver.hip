/*
 * ref_driver.hip -- extern "C" entry points into the upstream reference, built for gfx950.
 *
 * TEST INFRASTRUCTURE ONLY (tests/test_reference_gpu.py, tests/golden/make_reference_golden.py
 * through oracle/reference.py).  `make -C oracle ref` compiles this file together with the
 * hipified reference sources into oracle/_ref/libref_stixels.so; see oracle/Makefile and
 * oracle/ref_shim.h for the numerics substitutions.
 *
 * The driver calls the reference's own code and restates none of it:
 *   ref_stixels_compute  one frame through the reference's Stixels class in the call order of
 *                        apps/run_cityscapes.cu (SetConfig, Initialize, SetDisparityImage,
 *                        SetSegmentation, SetRoadParameters, Compute(pairwise), Finish) and
 *                        reads back the Sections, the joined disparity, the object LUT and the
 *                        instance-candidate arrays the class left on the device.
 *   ref_road_vdisparity  the three kernels of RoadEstimationKernels.cu with the launch geometry
 *                        of RoadEstimation::Compute.
 *   ref_road_*           the reference's RoadEstimation class itself: Initialize, Compute(host
 *                        image), the getters, Finish.  Its one call into OpenCV, cv::HoughLines,
 *                        lands in ref_stubs/opencv2/opencv.hpp, which holds no transform: it
 *                        records its arguments and returns the lines ref_road_set_lines installed.
 *
 * The reference's device asserts are compiled out (-DNDEBUG, as in its release build), so the
 * host checks below are what keep an input outside the reference's domain from
 * reaching a launch.  Segmentation values are not checked: StixelsKernel only sums, squares and
 * compares them (class costs, instance offsets); the one value it indexes with is the argmin
 * class of Cityscapes.h's fixed 19-class loops (semantic_class - 11 in [0, 8)).
 *
 * Stixels and RoadEstimation are opened with `private` read as `public` in this translation unit
 * only, to read the device buffers and the shape the classes keep (the layout does not change;
 * the reference is not edited).
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#define private public
#include "Stixels.hpp"
#include "RoadEstimation.h"
#undef private
#include "RoadEstimationKernels.h"

namespace {

std::string g_error;

enum {
    REF_OK = 0,
    REF_E_DOMAIN = 1,     // input outside the reference's domain: refused before any launch
    REF_E_HIP = 2,        // a HIP call or a reference launch failed
    REF_E_REFERENCE = 3,  // the reference reported an error (it prints and carries on)
    REF_E_OVERFLOW = 4,   // a column needed MAX_STIXELS_PER_COLUMN sections or more
};

int fail(int code, const std::string& what) {
    g_error = what;
    return code;
}

int hip_fail(const char* what, hipError_t e) {
    return fail(REF_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Captures what the reference writes to std::cerr (its launch errors) for the lifetime of the
// object; restores the stream on every exit path.
struct CerrCapture {
    std::ostringstream text;
    std::streambuf* saved;
    CerrCapture() : saved(std::cerr.rdbuf(text.rdbuf())) {}
    ~CerrCapture() { std::cerr.rdbuf(saved); }
};

int pow2_ceil_log2(int n) { return (int)powf(2, ceilf(log2f((float)n))); }  // as Stixels.cu

}  // namespace

extern "C" {

// Field for field the flat config of the project's host binding (_IshConfig, host.py).
struct ref_config {
    float rows, cols;
    int max_dis;
    float invalid_disparity, eps;
    int min_pts, size_filter, n_semantic_classes, n_offset_channels;
    float prior_weight, segmentation_weight, instance_weight, disparity_weight;
    int pairwise, column_step;
    float focal, baseline, camera_center_x, camera_center_y;
    float sigma_disparity_object, sigma_disparity_ground, sigma_sky;
    float pout, pout_sky, pord, pgrav, pblg;
    float pground_given_nexist, pobject_given_nexist, psky_given_nexist;
    float pnexist_dis, pground, pobject, psky;
    int width_margin;
    float sigma_camera_tilt, sigma_camera_height;
    int median_join;
    float epsilon, range_objects_z, road_vdisparity_threshold;
};

const char* ref_last_error() { return g_error.c_str(); }

int ref_max_sections() { return MAX_STIXELS_PER_COLUMN; }

// Shapes the reference derives from a config (Stixels.cu Initialize); -1 if the config is
// outside the domain.  out: realcols, rows_power2, rows_power2_segmentation, channels.
int ref_shapes(const ref_config* c, int* out) {
    const int rows = (int)c->rows, cols = (int)c->cols, D = c->max_dis;
    if ((float)rows != c->rows || (float)cols != c->cols)
        return fail(REF_E_DOMAIN, "rows / cols must be integers");
    if (c->column_step != DOWNSAMPLE_FACTOR)
        return fail(REF_E_DOMAIN, "column_step must be 8 (StixelsKernels.cu: assert DOWNSAMPLE_FACTOR == column_step)");
    if (D < 1 || rows < D)
        return fail(REF_E_DOMAIN, "need 1 <= max_dis <= rows (the kernel loads the disparity range with one thread per row)");
    if (rows > 1024)
        return fail(REF_E_DOMAIN, "rows > 1024: StixelsKernel launches one thread per row");
    if (3 * rows + 2 >= 32768)
        return fail(REF_E_DOMAIN, "3*rows + 2 must fit the int16 index table");
    if (c->n_semantic_classes != 19 || c->n_offset_channels != 2)
        return fail(REF_E_DOMAIN, "Cityscapes.h fixes 19 classes + 2 offset channels");
    if (c->width_margin < 0 || cols - c->width_margin < c->column_step)
        return fail(REF_E_DOMAIN, "no stixel column");
    out[0] = (cols - c->width_margin) / c->column_step;
    out[1] = pow2_ceil_log2(rows + 1);
    out[2] = pow2_ceil_log2(rows / 8 + 1);
    out[3] = c->n_semantic_classes + c->n_offset_channels;
    return REF_OK;
}

// One frame through the reference's Stixels class.  Inputs: disparity [rows][cols], segmentation
// [realcols][channels][rows_power2_segmentation] (not modified: Compute squares the offsets in
// place, SURVEY Q3, so the class works on its own copy).  Outputs (any may be null except
// sections): sections [realcols][MAX_STIXELS_PER_COLUMN] Section; joined [realcols][rows];
// object_lut [realcols][max_dis][rows_power2 + 1]; instance arrays [8][realcols * 200](x2) and
// per_class [8] in the reference's atomic arrival order; vhor_out the reference's vhor.
int ref_stixels_compute(const ref_config* c, int pairwise, const float* disparity,
                        const int32_t* segmentation, int vhor_image, float camera_tilt,
                        float camera_height, float alpha_ground, void* sections, float* joined,
                        float* object_lut, float* centerofmass, int32_t* indices, uint8_t* core,
                        int32_t* per_class, int* vhor_out) {
    int shp[4];
    if (int rc = ref_shapes(c, shp)) return rc;
    const int rows = (int)c->rows, cols = (int)c->cols, D = c->max_dis;
    const int C = shp[0], P2 = shp[1], P2S = shp[2], CH = shp[3];
    const int S = MAX_STIXELS_PER_COLUMN, K = 8;  // K: Stixels.cu m_instance_classes
    for (size_t i = 0, n = (size_t)rows * cols; i < n; ++i) {
        const float d = disparity[i];
        if (!(d >= 0.0f && d < (float)D))  // (also refuses NaN)
            return fail(REF_E_DOMAIN, "disparity " + std::to_string(d) + " at pixel " +
                                          std::to_string(i) + " is outside [0, max_dis)");
    }

    StixelConfig sc;
    sc.rows = c->rows; sc.cols = c->cols; sc.max_dis = c->max_dis;
    sc.invalid_disparity = c->invalid_disparity; sc.eps = c->eps; sc.min_pts = c->min_pts;
    sc.size_filter = c->size_filter; sc.n_semantic_classes = c->n_semantic_classes;
    sc.n_offset_channels = c->n_offset_channels; sc.prior_weight = c->prior_weight;
    sc.segmentation_weight = c->segmentation_weight; sc.instance_weight = c->instance_weight;
    sc.disparity_weight = c->disparity_weight; sc.pairwise = c->pairwise != 0;
    sc.column_step = c->column_step; sc.focal = c->focal; sc.baseline = c->baseline;
    sc.camera_center_x = c->camera_center_x; sc.camera_center_y = c->camera_center_y;
    sc.sigma_disparity_object = c->sigma_disparity_object;
    sc.sigma_disparity_ground = c->sigma_disparity_ground; sc.sigma_sky = c->sigma_sky;
    sc.pout = c->pout; sc.pout_sky = c->pout_sky; sc.pord = c->pord; sc.pgrav = c->pgrav;
    sc.pblg = c->pblg; sc.pground_given_nexist = c->pground_given_nexist;
    sc.pobject_given_nexist = c->pobject_given_nexist;
    sc.psky_given_nexist = c->psky_given_nexist; sc.pnexist_dis = c->pnexist_dis;
    sc.pground = c->pground; sc.pobject = c->pobject; sc.psky = c->psky;
    sc.width_margin = c->width_margin; sc.sigma_camera_tilt = c->sigma_camera_tilt;
    sc.sigma_camera_height = c->sigma_camera_height; sc.median_join = c->median_join != 0;
    sc.epsilon = c->epsilon; sc.range_objects_z = c->range_objects_z;
    sc.road_vdisparity_threshold = c->road_vdisparity_threshold;

    CerrCapture cap;
    Stixels st;
    try {
        st.SetConfig(sc);
    } catch (const std::exception& e) {
        return fail(REF_E_DOMAIN, std::string("SetConfig: ") + e.what());
    }
    st.Initialize();
    if (st.m_realcols != C || st.m_params.rows_power2 != P2 ||
        st.m_params.rows_power2_segmentation != P2S) {
        st.Finish();
        return fail(REF_E_DOMAIN, "the reference derived other shapes than ref_shapes");
    }

    // Bounds without the compiled-out `assert(i < params.max_sections)`: every section holds one
    // row or more, so a column writes at most rows + 1 entries from col * S on, and one class's
    // candidates number at most C * rows.  Reallocate the buffers the kernel fills to those
    // bounds (a column that needs S entries or more is reported as REF_E_OVERFLOW below).
    const size_t n_sec = (size_t)C * S + (size_t)rows + 1;
    const size_t n_inst = (size_t)K * C * S + (size_t)C * rows;
    hipError_t e = hipSuccess;
    for (void* p : {(void*)st.d_stixels, (void*)st.d_instance_centerofmass,
                    (void*)st.d_instance_labels, (void*)st.d_instance_indices,
                    (void*)st.d_instance_core_candidates})
        if (e == hipSuccess) e = hipFree(p);
    st.d_stixels = nullptr; st.d_instance_centerofmass = nullptr; st.d_instance_labels = nullptr;
    st.d_instance_indices = nullptr; st.d_instance_core_candidates = nullptr;
    if (e == hipSuccess) e = hipMalloc((void**)&st.d_stixels, n_sec * sizeof(Section));
    if (e == hipSuccess) e = hipMalloc((void**)&st.d_instance_centerofmass, n_inst * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&st.d_instance_labels, n_inst * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&st.d_instance_indices, n_inst * 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&st.d_instance_core_candidates, n_inst * sizeof(bool));
    if (e == hipSuccess) e = hipMemset(st.d_stixels, 0, n_sec * sizeof(Section));
    if (e == hipSuccess) e = hipMemset(st.d_instance_centerofmass, 0, n_inst * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(st.d_instance_indices, 0, n_inst * 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(st.d_instance_core_candidates, 0, n_inst * sizeof(bool));
    if (e != hipSuccess) {
        st.Finish();
        return hip_fail("instance / section buffers", e);
    }

    st.SetDisparityImage(std::vector<pixel_t>(disparity, disparity + (size_t)rows * cols));
    st.SetSegmentation(std::vector<int32_t>(segmentation, segmentation + (size_t)C * CH * P2S));
    st.SetRoadParameters(vhor_image, camera_tilt, camera_height, alpha_ground);
    StixelsData data;
    st.Compute(pairwise != 0, data);  // synchronises the device itself
    e = hipGetLastError();
    if (e != hipSuccess) {
        st.Finish();
        return hip_fail("reference Compute", e);
    }
    if (!cap.text.str().empty()) {
        st.Finish();
        return fail(REF_E_REFERENCE, "the reference reported: " + cap.text.str());
    }

    std::memcpy(sections, data.sections.data(), (size_t)C * S * sizeof(Section));
    if (joined)
        e = hipMemcpy(joined, st.d_disparity, (size_t)C * rows * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && object_lut)
        e = hipMemcpy(object_lut, st.d_object_lut, (size_t)C * D * (P2 + 1) * sizeof(float),
                      hipMemcpyDeviceToHost);
    if (e == hipSuccess && centerofmass)
        e = hipMemcpy(centerofmass, st.d_instance_centerofmass, (size_t)K * C * S * 2 * sizeof(float),
                      hipMemcpyDeviceToHost);
    if (e == hipSuccess && indices)
        e = hipMemcpy(indices, st.d_instance_indices, (size_t)K * C * S * 2 * sizeof(int32_t),
                      hipMemcpyDeviceToHost);
    if (e == hipSuccess && core) {
        static_assert(sizeof(bool) == 1, "bool is one byte");
        e = hipMemcpy(core, st.d_instance_core_candidates, (size_t)K * C * S, hipMemcpyDeviceToHost);
    }
    if (e == hipSuccess && per_class)
        e = hipMemcpy(per_class, st.d_instances_per_class, K * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (vhor_out) *vhor_out = st.m_vhor;
    st.Finish();
    if (e != hipSuccess) return hip_fail("read-back", e);

    const Section* sec = static_cast<const Section*>(sections);
    for (int col = 0; col < C; ++col) {
        bool terminated = false;
        for (int i = 0; i < S && !terminated; ++i) terminated = sec[(size_t)col * S + i].type == -1;
        if (!terminated)
            return fail(REF_E_OVERFLOW, "column " + std::to_string(col) + " has no terminator within " +
                                            std::to_string(S) + " sections");
    }
    return REF_OK;
}

// The v-disparity histogram, its maximum and the binary image of RoadEstimation::Compute
// (RoadEstimation.cu, the three launches before the Hough transform).  disparity [rows][cols];
// vdisp [rows][max_dis] int32, binary [rows][max_dis] uint8, maximum one int32.
int ref_road_vdisparity(const float* disparity, int rows, int cols, int max_dis, float threshold,
                        int32_t* vdisp, uint8_t* binary, int32_t* maximum) {
    if (rows < 1 || cols < 1 || max_dis < 1)
        return fail(REF_E_DOMAIN, "empty frame");
    const size_t n = (size_t)rows * cols, nv = (size_t)rows * max_dis;
    for (size_t i = 0; i < n; ++i)  // ComputeHistogram indexes with (int) d for every d != 0
        if (!(disparity[i] >= 0.0f && disparity[i] < (float)max_dis))
            return fail(REF_E_DOMAIN, "disparity outside [0, max_dis) at pixel " + std::to_string(i));
    pixel_t* d_disparity = nullptr;
    int *d_vdisp = nullptr, *d_maximum = nullptr;
    uint8_t* d_binary = nullptr;
    int rc = REF_OK;
    hipError_t e = hipMalloc((void**)&d_disparity, n * sizeof(pixel_t));
    if (e == hipSuccess) e = hipMalloc((void**)&d_vdisp, nv * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&d_maximum, sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&d_binary, nv);
    if (e == hipSuccess) e = hipMemcpy(d_disparity, disparity, n * sizeof(pixel_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_maximum, 0, sizeof(int));
    if (e == hipSuccess) e = hipMemset(d_vdisp, 0, nv * sizeof(int));
    if (e != hipSuccess) rc = hip_fail("road buffers", e);
    if (rc == REF_OK) {
        ComputeHistogram<<<(rows * cols + 256 - 1) / 256, 256>>>(d_disparity, d_vdisp, rows, cols, max_dis);
        if ((e = hipGetLastError()) != hipSuccess) rc = hip_fail("ComputeHistogram", e);
    }
    if (rc == REF_OK) {
        ComputeMaximum<<<(rows * max_dis + 256 - 1) / 256, 256>>>(d_vdisp, d_maximum, rows, max_dis);
        if ((e = hipGetLastError()) != hipSuccess) rc = hip_fail("ComputeMaximum", e);
    }
    if (rc == REF_OK) {
        ComputeBinaryImage<<<(rows * max_dis + 256 - 1) / 256, 256>>>(d_vdisp, d_binary, d_maximum,
                                                                       threshold, rows, max_dis);
        if ((e = hipGetLastError()) != hipSuccess) rc = hip_fail("ComputeBinaryImage", e);
    }
    if (rc == REF_OK && (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail("road kernels", e);
    if (rc == REF_OK && (e = hipMemcpy(vdisp, d_vdisp, nv * sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess)
        rc = hip_fail("read-back", e);
    if (rc == REF_OK && (e = hipMemcpy(binary, d_binary, nv, hipMemcpyDeviceToHost)) != hipSuccess)
        rc = hip_fail("read-back", e);
    if (rc == REF_OK && (e = hipMemcpy(maximum, d_maximum, sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess)
        rc = hip_fail("read-back", e);
    for (void* p : {(void*)d_disparity, (void*)d_vdisp, (void*)d_maximum, (void*)d_binary})
        if (p) (void)hipFree(p);
    return rc;
}

// ---- the reference's RoadEstimation class ------------------------------------------------------
// One object per handle.  The class neither checks its shape nor the bins it counts into, so
// initialize and compute check them here, as ref_road_vdisparity does.

int ref_road_create(void** out) {
    *out = new RoadEstimation();
    return REF_OK;
}

int ref_road_finish(void* h) {
    RoadEstimation* re = static_cast<RoadEstimation*>(h);
    if (re->IsInitialized()) re->Finish();
    return REF_OK;
}

int ref_road_destroy(void* h) {
    if (!h) return REF_OK;
    ref_road_finish(h);
    delete static_cast<RoadEstimation*>(h);
    return REF_OK;
}

// Initialize; an initialised object is finished first (the class itself would leak its buffers),
// which is what the reference's wrapper does before it initialises for another shape.
int ref_road_initialize(void* h, float camera_center_y, float baseline, float focal, int rows, int cols,
                        int max_dis, float threshold) {
    if (rows < 1 || cols < 1 || max_dis < 1) return fail(REF_E_DOMAIN, "empty frame");
    RoadEstimation* re = static_cast<RoadEstimation*>(h);
    ref_road_finish(h);
    re->Initialize(camera_center_y, baseline, focal, rows, cols, max_dis, threshold);
    return REF_OK;
}

// The lines the stub's cv::HoughLines returns from now on: lines [n][2] (rho, theta).
int ref_road_set_lines(const float* lines, int n) {
    std::vector<cv::Vec2f>& a = cv::hough_lines_stub().answer;
    a.resize((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; ++i) {
        a[i][0] = lines[2 * i];
        a[i][1] = lines[2 * i + 1];
    }
    return REF_OK;
}

// RoadEstimation::Compute(const std::vector<pixel_t>&) on disparity [rows][cols]; *ok: its return value.
int ref_road_compute(void* h, const float* disparity, size_t n, int* ok) {
    RoadEstimation* re = static_cast<RoadEstimation*>(h);
    if (!re->IsInitialized()) return fail(REF_E_DOMAIN, "RoadEstimation is not initialised");
    if (n != (size_t)re->m_rows * re->m_cols) return fail(REF_E_DOMAIN, "the image is not rows x cols");
    for (size_t i = 0; i < n; ++i)  // ComputeHistogram indexes with (int) d for every d != 0
        if (!(disparity[i] >= 0.0f && disparity[i] < (float)re->m_max_dis))
            return fail(REF_E_DOMAIN, "disparity outside [0, max_dis) at pixel " + std::to_string(i));
    const bool found = re->Compute(std::vector<pixel_t>(disparity, disparity + n));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail("reference RoadEstimation::Compute", e);
    *ok = found ? 1 : 0;
    return REF_OK;
}

// out5: pitch, camera height, slope, and the (|rho|, theta) of the line the class accepted last
int ref_road_get(void* h, int* horizon_point, float* out5) {
    RoadEstimation* re = static_cast<RoadEstimation*>(h);
    *horizon_point = re->GetHorizonPoint();
    out5[0] = re->GetPitch();
    out5[1] = re->GetCameraHeight();
    out5[2] = re->GetSlope();
    out5[3] = re->m_rho;
    out5[4] = re->m_theta;
    return REF_OK;
}

// What the stub's cv::HoughLines saw last.  ints: rows, cols, type, threshold, calls so far;
// doubles: rho, theta; image (may be null): up to n bytes of its copy of the image.
int ref_road_hough_call(int* ints, double* doubles, uint8_t* image, size_t n) {
    const cv::HoughLinesStub& s = cv::hough_lines_stub();
    ints[0] = s.rows; ints[1] = s.cols; ints[2] = s.type; ints[3] = s.threshold; ints[4] = s.calls;
    doubles[0] = s.rho; doubles[1] = s.theta;
    if (image) {
        if (n != s.image.size()) return fail(REF_E_DOMAIN, "the recorded image has another size");
        std::memcpy(image, s.image.data(), n);
    }
    return REF_OK;
}

}  // extern "C"
