/*
 * Stixels.cpp -- host class of the MI355X-native stixel library (plain C++, no HIP headers).
 *
 * Mirrors the behaviour of the reference's host driver
 * (/root/reference/InstanceStixels/src/Stixels.cu:33-926) on top of the C ABI in
 * include/instance_stixels_core.h: same setters, same frame-independent precompute
 * (Initialize), same per-frame ground model (PrecomputeGround), same Compute() call sequence
 * and error conventions (std::invalid_argument for unset configuration, message + exit(1) for
 * device runtime failures).  Citations `Stixels.cu:N` refer to that file.
 */
#include "InstanceStixels/Stixels.hpp"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <thread>

#include "DeviceGuard.h"
#include "is_ground_model.h"

Stixels::Stixels() {}
Stixels::~Stixels() {} /* like the reference, buffers are released by Finish(), Stixels.cu:36-37 */

/* ---------------------------------------------------------------- configuration setters */

void Stixels::SetConfig(const StixelConfig& config) { /* Stixels.cu:292-338 */
    if (config.rows == -1 || config.cols == -1)
        throw std::invalid_argument("Number of rows or columns are not set.");
    if (config.max_dis == -1) throw std::invalid_argument("Maximum disparity value is not set.");
    if (config.eps == -1 || config.min_pts == -1 || config.size_filter == -1)
        throw std::invalid_argument("Clustering parameters are not set.");
    if (config.prior_weight == -1 || config.segmentation_weight == -1 ||
        config.instance_weight == -1 || config.disparity_weight == -1)
        throw std::invalid_argument("Energy term weights are not set.");
    if (config.column_step == -1) throw std::invalid_argument("Stixel width is not set.");
    if (config.focal == -1 || config.baseline == -1)
        throw std::invalid_argument("Camera parameters are not set.");

    SetDisparityParameters(config.rows, config.cols, config.max_dis, config.invalid_disparity,
                           config.sigma_disparity_object, config.sigma_disparity_ground,
                           config.sigma_sky);
    SetSegmentationParameters(config.n_semantic_classes, config.n_offset_channels);
    SetClusteringParameters(config.eps, config.min_pts, config.size_filter);
    SetWeightParameters(config.prior_weight, config.disparity_weight, config.segmentation_weight,
                        config.instance_weight);
    SetProbabilities(config.pout, config.pout_sky, config.pground_given_nexist,
                     config.pobject_given_nexist, config.psky_given_nexist, config.pnexist_dis,
                     config.pground, config.pobject, config.psky, config.pord, config.pgrav,
                     config.pblg);
    SetModelParameters(config.column_step, config.median_join, config.epsilon,
                       config.range_objects_z, config.width_margin);
    SetCameraParameters(config.focal, config.baseline, config.sigma_camera_tilt,
                        config.sigma_camera_height, config.camera_center_x,
                        config.camera_center_y);
}

void Stixels::SetProbabilities(float pout, float pout_sky, float pground_given_nexist,
                               float pobject_given_nexist, float psky_given_nexist,
                               float pnexist_dis, float pground, float pobject, float psky,
                               float pord, float pgrav, float pblg) { /* Stixels.cu:361-373 */
    m_pout = pout;
    m_pout_sky = pout_sky;
    m_pnexists_given_ground = (pground_given_nexist * pnexist_dis) / pground;
    m_pnexists_given_object = (pobject_given_nexist * pnexist_dis) / pobject;
    m_pnexists_given_sky = (psky_given_nexist * pnexist_dis) / psky;
    m_pord = pord;
    m_pgrav = pgrav;
    m_pblg = pblg;
}

void Stixels::SetRoadParameters(int vhor, float camera_tilt, float camera_height,
                                float alpha_ground) { /* Stixels.cu:375-381 */
    m_vhor = m_rows - vhor - 1;
    m_camera_tilt = camera_tilt;
    m_camera_height = camera_height;
    m_alpha_ground = alpha_ground;
}

void Stixels::SetCameraParameters(float focal, float baseline, float sigma_camera_tilt,
                                  float sigma_camera_height, float camera_center_x,
                                  float camera_center_y) { /* Stixels.cu:383-393 */
    m_focal = focal;
    m_baseline = baseline;
    m_sigma_camera_tilt = sigma_camera_tilt * (PIFLOAT) / 180.0f; /* degrees -> radians */
    m_sigma_camera_height = sigma_camera_height;
    m_camera_center_x = camera_center_x;
    m_camera_center_y = camera_center_y;
}

void Stixels::SetClusteringParameters(const float eps, const int min_pts,
                                      const int size_filter) { /* Stixels.cu:395-400 */
    m_params.clustering_eps = eps;
    m_params.clustering_min_pts = min_pts;
    m_params.clustering_size_filter = size_filter;
}

void Stixels::SetSegmentationParameters(const int classes,
                                        const int instance_channels) { /* Stixels.cu:402-406 */
    m_segmentation_classes = classes;
    m_segmentation_channels = classes + instance_channels;
}

void Stixels::SetWeightParameters(const float prior_weight, const float disparity_weight,
                                  const float segmentation_weight,
                                  const float instance_weight) { /* Stixels.cu:408-423 */
    m_prior_weight = prior_weight;
    m_disparity_weight = disparity_weight;
    m_segmentation_weight = segmentation_weight;
    /* the instance weight is expressed relative to the segmentation weight */
    m_instance_weight = 0.0;
    if (segmentation_weight > 1e-5) {
        m_instance_weight = instance_weight / segmentation_weight;
        if (instance_weight < 1e-8) m_instance_weight = 0.0;
    }
}

void Stixels::SetDisparityParameters(const int rows, const int cols, const int max_dis,
                                     const float invalid_disparity,
                                     const float sigma_disparity_object,
                                     const float sigma_disparity_ground,
                                     const float sigma_sky) { /* Stixels.cu:425-437 */
    m_rows = rows;
    m_cols = cols;
    m_max_dis = max_dis;
    m_max_disf = (float)m_max_dis;
    m_sigma_disparity_object = sigma_disparity_object;
    m_sigma_disparity_ground = sigma_disparity_ground;
    m_sigma_sky = sigma_sky;
    m_invalid_disparity = invalid_disparity;
}

void Stixels::SetModelParameters(const int column_step, const bool median_join, float epsilon,
                                 float range_objects_z, int width_margin) { /* Stixels.cu:439-446 */
    m_column_step = column_step;
    m_median_join = median_join;
    m_epsilon = epsilon;
    m_range_objects_z = range_objects_z;
    m_width_margin = width_margin;
}

/* ---------------------------------------------------------------- precompute */

float Stixels::FastLog(float v) const { /* Stixels.cu:786-788 */
    return m_log_lut[(int)((v)*LOG_LUT_SIZE + 0.5f)];
}

float Stixels::ComputeObjectDisparityRange(const float previous_mean) const { /* :879-887 */
    float range_disp = 0.0f;
    if (previous_mean != 0) {
        const float pmean_plus_z = (m_baseline * m_focal / previous_mean) + m_range_objects_z;
        range_disp = previous_mean - (m_baseline * m_focal / pmean_plus_z);
    }
    return range_disp;
}

void Stixels::PrecomputeSky() { /* Stixels.cu:856-865 */
    const float sigma = m_sigma_sky;
    const float pout = m_pout_sky;
    const float a_range =
        0.5f * (std::erf(m_max_disf / (sigma * sqrtf(2.0f))) - std::erf(0.0f));
    m_normalization_sky =
        FastLog(a_range) - logf((1.0f - pout) / (sigma * sqrtf(2.0f * PIFLOAT)));
    m_inv_sigma2_sky = 1.0f / (2.0f * sigma * sigma);
}

void Stixels::PrecomputeObject() { /* Stixels.cu:819-840 */
    const float pout = m_pout;
    m_normalization_object.assign(m_max_dis, 0.0f);
    m_inv_sigma2_object.assign(m_max_dis, 0.0f);
    for (int dis = 0; dis < m_max_dis; dis++) {
        const float fn = (float)dis;
        const float sigma_object = fn * fn * m_range_objects_z / (m_focal * m_baseline);
        const float sigma = sqrtf(m_sigma_disparity_object * m_sigma_disparity_object +
                                  sigma_object * sigma_object);
        const float a_range = 0.5f * (std::erf((m_max_disf - fn) / (sigma * sqrtf(2.0f))) -
                                      std::erf((-fn) / (sigma * sqrtf(2.0f))));
        m_normalization_object[dis] =
            FastLog(a_range) - FastLog((1.0f - pout) / (sigma * sqrtf(2.0f * PIFLOAT)));
        m_inv_sigma2_object[dis] = 1.0f / (2.0f * sigma * sigma);
    }
}

float Stixels::GetDataCostObject(const int fn, const int dis) const { /* Stixels.cu:842-854 */
    float data_cost = m_params.pnexists_given_object_log;
    if (dis != (int)m_invalid_disparity) {
        const float model_diff = (float)(dis - fn);
        const float pgaussian =
            m_normalization_object[fn] + model_diff * model_diff * m_inv_sigma2_object[fn];
        const float p_data = fminf(m_puniform, pgaussian);
        data_cost = p_data + m_params.nopnexists_given_object_log;
    }
    return data_cost;
}

void Stixels::PrecomputeGround(int vhor_lib, float camera_tilt, float camera_height,
                               float alpha_ground, GroundModel& out) const { /* :790-817 */
    const float fb = (m_focal * m_baseline) / camera_height;
    const float pout = m_pout;
    out.function.resize(m_rows);
    out.normalization.resize(m_rows);
    out.inv_sigma2.resize(m_rows);
    for (int v = 0; v < m_rows; v++) {
        const float fn = alpha_ground * (float)(vhor_lib - v); /* GroundFunction, :867-877 */
        out.function[v] = fn;
        const float x = camera_tilt + (float)(vhor_lib - v) / m_focal;
        const float sigma2_road =
            fb * fb *
            (m_sigma_camera_height * m_sigma_camera_height * x * x /
                 (camera_height * camera_height) +
             m_sigma_camera_tilt * m_sigma_camera_tilt);
        const float sigma =
            sqrtf(m_sigma_disparity_ground * m_sigma_disparity_ground + sigma2_road);
        const float a_range = 0.5f * (std::erf((m_max_disf - fn) / (sigma * sqrtf(2.0f))) -
                                      std::erf((-fn) / (sigma * sqrtf(2.0f))));
        out.normalization[v] =
            FastLog(a_range) - FastLog((1.0f - pout) / (sigma * sqrtf(2.0f * PIFLOAT)));
        out.inv_sigma2[v] = 1.0f / (2.0f * sigma * sigma);
    }
}

is_ground_params Stixels::GroundParams() const {
    return is_ground_params{m_focal, m_baseline, m_max_disf, m_pout, m_sigma_disparity_ground, m_sigma_camera_height,
                            m_sigma_camera_tilt};
}

void Stixels::PrecomputeGroundShared(const is_ground_params& g, const float* log_lut, int lut_entries, int rows,
                                     int vhor_lib, float camera_tilt, float camera_height, float alpha_ground,
                                     float* function, float* normalization, float* inv_sigma2, int* range_index) {
    for (int v = 0; v < rows; v++)
        is_ground_row(&g, log_lut, lut_entries, vhor_lib, camera_tilt, camera_height, alpha_ground, v, function + v,
                      normalization + v, inv_sigma2 + v, range_index ? range_index + v : nullptr);
}

void Stixels::GetGroundModel(std::vector<float>& ground_function,
                             std::vector<float>& normalization_ground,
                             std::vector<float>& inv_sigma2_ground, int& vhor_lib) {
    GroundModel g;
    PrecomputeGround(m_vhor, m_camera_tilt, m_camera_height, m_alpha_ground, g);
    ground_function = g.function;
    normalization_ground = g.normalization;
    inv_sigma2_ground = g.inv_sigma2;
    vhor_lib = m_vhor;
}

/* ---------------------------------------------------------------- Initialize / Finish */

void Stixels::Initialize() { InitializeBatch(1); }

/* Host half of Initialize: every frame-independent table and the kernel parameter block
 * (Stixels.cu:44-47, 79-133, 212-245).  Needs no device. */
void Stixels::PrecomputeHost() {
    m_realcols = (m_cols - m_width_margin) / m_column_step;
    m_max_sections = MAX_STIXELS_PER_COLUMN;
    m_instance_classes = IS_INSTANCE_CLASSES;

    m_instances_per_class.assign(m_instance_classes, 0);

    /* log LUT over [0, 1], Stixels.cu:79-84 */
    m_log_lut.resize(LOG_LUT_SIZE + 1);
    for (int i = 0; i < LOG_LUT_SIZE; i++) {
        const float log_res = (float)i / ((float)LOG_LUT_SIZE);
        m_log_lut[i] = logf(log_res);
    }
    m_log_lut[LOG_LUT_SIZE] = 0.0f;

    /* frequently used values, Stixels.cu:93-102 */
    m_max_dis_log = logf(m_max_disf);
    m_rows_log = logf((float)m_rows);
    m_puniform_sky = m_max_dis_log - logf(m_pout_sky);
    m_puniform = m_max_dis_log - logf(m_pout);
    m_params.pnexists_given_sky_log = -logf(m_pnexists_given_sky);
    m_params.nopnexists_given_sky_log = -logf(1.0f - m_pnexists_given_sky);
    m_params.pnexists_given_ground_log = -logf(m_pnexists_given_ground);
    m_params.nopnexists_given_ground_log = -logf(1.0f - m_pnexists_given_ground);
    m_params.pnexists_given_object_log = -logf(m_pnexists_given_object);
    m_params.nopnexists_given_object_log = -logf(1.0f - m_pnexists_given_object);

    m_object_disparity_range.resize(m_max_dis);
    for (int i = 0; i < m_max_dis; i++)
        m_object_disparity_range[i] = ComputeObjectDisparityRange((float)i); /* :111-115 */

    PrecomputeSky();
    PrecomputeObject();

    m_obj_cost_lut.resize((size_t)m_max_dis * m_max_dis); /* :122-129 */
    for (int fn = 0; fn < m_max_dis; fn++)
        for (int dis = 0; dis < m_max_dis; dis++)
            m_obj_cost_lut[(size_t)fn * m_max_dis + dis] = GetDataCostObject(fn, dis);

    const int rows_power2 = (int)powf(2, ceilf(log2f(m_rows + 1))); /* :131-133 */
    const int rows_power2_segmentation = (int)powf(2, ceilf(log2f(m_rows / 8 + 1)));

    /* kernel parameter block, Stixels.cu:212-245 */
    m_params.vhor = 0;
    m_params.rows = m_rows;
    m_params.cols = m_realcols;
    m_params.max_dis = m_max_dis;
    m_params.invalid_disparity = m_invalid_disparity;
    m_params.rows_log = m_rows_log;
    m_params.normalization_sky = m_normalization_sky;
    m_params.inv_sigma2_sky = m_inv_sigma2_sky;
    m_params.puniform_sky = m_puniform_sky;
    m_params.puniform = m_puniform;
    m_params.baseline = m_baseline;
    m_params.focal = m_focal;
    m_params.range_objects_z = m_range_objects_z;
    m_params.pord = m_pord;
    m_params.epsilon = m_epsilon;
    m_params.pgrav = m_pgrav;
    m_params.pblg = m_pblg;
    m_params.rows_power2 = rows_power2;
    m_params.rows_power2_segmentation = rows_power2_segmentation;
    m_params.max_sections = m_max_sections;
    m_params.max_dis_log = m_max_dis_log;
    m_params.width_margin = m_width_margin;
    m_params.segmentation_classes = m_segmentation_classes;
    m_params.segmentation_channels = m_segmentation_channels;
    m_params.prior_weight = m_prior_weight;
    m_params.disparity_weight = m_disparity_weight;
    m_params.segmentation_weight = m_segmentation_weight;
    m_params.instance_weight = m_instance_weight;
    m_params.column_step = m_column_step;
}

void Stixels::InitializeBatch(int max_batch) { /* Stixels.cu:43-248 */
    m_max_batch = std::max(1, max_batch);
    PrecomputeHost();
    const size_t inst_n = (size_t)m_instance_classes * m_realcols * m_max_sections;
    const int rows_power2_segmentation = m_params.rows_power2_segmentation;

    /* device side: LUT upload + all buffers (Stixels.cu:53-74, 136-210) on the caller's current
     * device unless SetDevice() chose one */
    int device = m_device;
    if (device < 0) IS_CHECK_RETURN(is_get_device(&device));
    m_ctx_device = device; /* (m_device keeps the REQUEST: -1 resolves again at the next Initialize) */
    const DeviceGuard guard(device);
    IS_CHECK_RETURN(is_ctx_create(&m_params, m_obj_cost_lut.data(),
                                  m_object_disparity_range.data(), m_max_batch, device, &m_ctx));
    IS_CHECK_RETURN(is_stream_create(&m_stream, 1));
    const size_t B = m_max_batch;
    /* [header rows: per-class counts][B x C x S sections]: one pitched copy fetches both */
    const size_t row_bytes = (size_t)m_max_sections * sizeof(Section);
    m_header_rows = (int)((B * m_instance_classes * sizeof(int32_t) + row_bytes - 1) / row_bytes);
    m_head_sections = m_max_sections < 64 ? m_max_sections : 64;
    d_stixels_block.reserve(((size_t)m_header_rows + B * m_realcols) * m_max_sections);
    d_stixels = d_stixels_block.get() + (size_t)m_header_rows * m_max_sections;
    d_instances_per_class = reinterpret_cast<int32_t*>(d_stixels_block.get());
    d_instance_centerofmass.reserve(B * inst_n * 2);
    d_instance_indices.reserve(B * inst_n * 2);
    d_instance_core_candidates.reserve(B * inst_n);
    d_segmentation.reserve((size_t)rows_power2_segmentation * m_realcols * m_segmentation_channels);
    d_disparity_big.reserve((size_t)m_rows * m_cols);
    d_disparity.reserve(B * m_rows * m_realcols);
    d_instance_labels.reserve(B * inst_n);
    d_instance_packed.reserve(B * (1 + 3 * inst_n));
    h_stixels.reserve((size_t)m_realcols * m_max_sections);
    h_stixels_head.reserve(((size_t)m_header_rows + m_realcols) * m_head_sections);
    h_instance_head.reserve(B * 16);
    h_instance_packed.reserve(1 + 3 * inst_n);
    h_instance_packed.get()[0] = 0;
    /* ComputeBatchRoad: the constants and the FastLog table of the device ground model, once per context */
    const is_ground_params gp = GroundParams();
    IS_CHECK_RETURN(is_ctx_set_ground_model(m_ctx, &gp, m_log_lut.data(), (int)m_log_lut.size()));
    h_road.reserve(B * (sizeof(RoadParameters) + 1));
    m_road_vhor_hint = -1;
    m_ground_valid = false; /* (the ground model depends on the configuration just applied) */
    m_is_initialized = true;
}

void Stixels::Finish() { /* Stixels.cu:250-283 */
    const DeviceGuard guard(m_ctx_device);
    release_all();
    d_stixels = nullptr; d_instances_per_class = nullptr; /* (aliases into d_stixels_block) */
    m_objects_cap = m_object_points_cap = 0;
    ForgetBatch();
    IS_CHECK_RETURN(is_ctx_destroy(m_ctx));
    m_ctx = nullptr;
    IS_CHECK_RETURN(is_stream_destroy(m_stream));
    m_stream = nullptr;
    m_log_lut.clear(); m_obj_cost_lut.clear(); m_object_disparity_range.clear();
    m_normalization_object.clear(); m_inv_sigma2_object.clear();
    m_is_initialized = false;
    m_ctx_device = -1;
}

/* ---------------------------------------------------------------- per-frame inputs */

void Stixels::SetSegmentation(const std::vector<int32_t>& segmentation) { /* :340-346 */
    const DeviceGuard guard(m_ctx_device);
    IS_CHECK_RETURN(is_memcpy_h2d(d_segmentation.get(), segmentation.data(),
                                  sizeof(int32_t) * segmentation.size(), m_stream));
    IS_CHECK_RETURN(is_stream_synchronize(m_stream));
}

void Stixels::SetDisparityImage(const std::vector<pixel_t>& disp_im) { /* :348-355 */
    const DeviceGuard guard(m_ctx_device);
    /* the reference queues a cudaMemcpyAsync from the caller's pageable vector; the copy is
     * finished here before returning, so the vector may be a temporary */
    IS_CHECK_RETURN(is_memcpy_h2d(d_disparity_big.get(), disp_im.data(),
                                  sizeof(pixel_t) * disp_im.size(), m_stream));
    IS_CHECK_RETURN(is_stream_synchronize(m_stream));
}

pixel_t* Stixels::GetInputDisparityImageOnDevice() { return d_disparity_big.get(); } /* :357-359 */
int Stixels::GetRealCols() { return m_realcols; }
int Stixels::GetMaxSections() { return m_max_sections; }

/* ---------------------------------------------------------------- Compute */

void Stixels::FillHeader(StixelsData& d, float alpha_ground, int vhor_lib) const { /* :615-627 */
    d.sections.resize((size_t)m_realcols * m_max_sections);
    d.rows = m_rows;
    d.cols = m_cols;
    d.realcols = m_realcols;
    d.max_sections = m_max_sections;
    d.max_dis = m_max_dis;
    d.column_step = m_column_step;
    d.semantic_classes = m_segmentation_classes;
    d.alpha_ground = alpha_ground;
    d.vhor = vhor_lib;
}

float Stixels::Compute(const bool pairwise, StixelsData& stixels_data,
                       int32_t* d_segmentation_local) { /* Stixels.cu:449-637 */
    if (d_segmentation_local == nullptr) d_segmentation_local = d_segmentation.get();
    const DeviceGuard guard(m_ctx_device);

    /* JoinColumns does not need the ground model: it runs while the host computes it */
    IS_CHECK_RETURN(is_join_columns(m_ctx, d_disparity_big.get(), m_cols, m_median_join ? 1 : 0,
                                    d_disparity.get(), 1, m_stream)); /* :509-511 */
    GroundModel& g = m_ground;
    const float key[12] = {(float)m_vhor, m_camera_tilt, m_camera_height, m_alpha_ground, m_focal, m_baseline,
                           m_pout, m_sigma_camera_height, m_sigma_camera_tilt, m_sigma_disparity_ground,
                           m_max_disf, (float)m_rows};
    /* (memcmp: a NaN parameter compares equal to itself here, the model it gives is the same) */
    if (!m_ground_valid || std::memcmp(key, m_ground_key, sizeof(key)) != 0) {
        PrecomputeGround(m_vhor, m_camera_tilt, m_camera_height, m_alpha_ground, g); /* :463 */
        std::memcpy(m_ground_key, key, sizeof(key));
        m_ground_valid = true;
    }
    m_params.vhor = m_vhor;                                                       /* :532 */
    /* the DP, the instance candidates and their clustering (ClusterInstances, :613) are queued
     * back to back on the device; nothing returns to the host in between */
    const is_instance_buffers ib = InstanceBuffers(0);
    IS_CHECK_RETURN(is_compute(m_ctx, d_disparity.get(), d_segmentation_local, g.function.data(),
                               g.normalization.data(), g.inv_sigma2.data(), &m_vhor,
                               pairwise ? 1 : 0, 1, d_stixels, &ib, nullptr, nullptr,
                               m_stream)); /* :535-590 */
    RememberBatch(1, true, &m_alpha_ground, &m_vhor);
    /* results into pinned memory, ONE copy and ONE synchronisation (:600, :629-633): the header
     * row(s) with the per-class counts and the first m_head_sections sections of every column (a
     * column rarely has more: 10-40 on road scenes) */
    const int K = m_head_sections;
    const size_t row_bytes = (size_t)m_max_sections * sizeof(Section);
    IS_CHECK_RETURN(is_memcpy2d_d2h(h_stixels_head.get(), (size_t)K * sizeof(Section), d_stixels_block.get(), row_bytes,
                                    (size_t)K * sizeof(Section), (size_t)m_header_rows + m_realcols,
                                    m_stream));
    IS_CHECK_RETURN(is_stream_synchronize(m_stream));
    const int32_t* head = reinterpret_cast<const int32_t*>(h_stixels_head.get());
    for (int k = 0; k < m_instance_classes; k++) m_instances_per_class[k] = head[k];
    m_labels_on_host = false;

    FillHeader(stixels_data, m_alpha_ground, m_vhor);
    /* sections of every column up to and including its terminator; what lies behind a
     * terminator is unspecified (in the reference: whatever the device buffer held) */
    Section* out = stixels_data.sections.data();
    const Section* cols = h_stixels_head.get() + (size_t)m_header_rows * K;
    bool complete = true;
    for (int c = 0; c < m_realcols && complete; c++) {
        const Section* src = cols + (size_t)c * K;
        int n = 0;
        while (n < K && src[n].type != -1) n++;
        if (n == K && K < m_max_sections) { complete = false; break; } /* no terminator among the first K */
        if (n == K) n = K - 1; /* (K == max_sections: the last slot ends the column, as below) */
        std::memcpy(out + (size_t)c * m_max_sections, src, (size_t)(n + 1) * sizeof(Section));
    }
    if (!complete) { /* a column with more than K sections: fetch everything */
        const size_t n_sec = (size_t)m_realcols * m_max_sections;
        IS_CHECK_RETURN(is_memcpy_d2h(h_stixels.get(), d_stixels, n_sec * sizeof(Section), m_stream));
        IS_CHECK_RETURN(is_stream_synchronize(m_stream));
        for (int c = 0; c < m_realcols; c++) {
            const Section* src = h_stixels.get() + (size_t)c * m_max_sections;
            int n = 0;
            while (n < m_max_sections - 1 && src[n].type != -1) n++;
            std::memcpy(out + (size_t)c * m_max_sections, src, (size_t)(n + 1) * sizeof(Section));
        }
    }
    return -1; /* the reference's timers are commented out, Stixels.cu:636 */
}

/* what the consumers read: the arrays of the last compute call, or of the selected set of a sweep (the compute calls
 * themselves always write the object's own arrays, InstanceBuffers) */
is_instance_buffers Stixels::LastInstanceBuffers(int image) const {
    return m_sweep.sets > 0 ? SweepInstanceBuffers(m_sweep.selected, image) : InstanceBuffers(image);
}

is_instance_buffers Stixels::InstanceBuffers(int image) const {
    const size_t inst_n = (size_t)m_instance_classes * m_realcols * m_max_sections;
    const size_t i = (size_t)image;
    is_instance_buffers ib = {}; /* (zero-initialised: fields added by later versions stay NULL) */
    ib.d_centerofmass = d_instance_centerofmass.get() + i * inst_n * 2;
    ib.d_indices = d_instance_indices.get() + i * inst_n * 2;
    ib.d_core_candidates = d_instance_core_candidates.get() + i * inst_n;
    ib.d_instances_per_class = d_instances_per_class + i * m_instance_classes;
    ib.d_labels = d_instance_labels.get() + i * inst_n;
    ib.d_packed = d_instance_packed.get() + i * (1 + 3 * inst_n);
    return ib;
}

/* the ground model of every frame of a batch on the host (the DP reads it from the core's staging block) */
void Stixels::BatchGround(int n_images, const RoadParameters* road, GroundModel& batch,
                          std::vector<int>& vhor) const {
    const size_t H = (size_t)m_rows;
    batch.function.resize(n_images * H);
    batch.normalization.resize(n_images * H);
    batch.inv_sigma2.resize(n_images * H);
    vhor.resize(n_images);
    GroundModel g;
    for (int i = 0; i < n_images; i++) {
        vhor[i] = m_rows - road[i].vhor - 1;
        PrecomputeGround(vhor[i], road[i].camera_tilt, road[i].camera_height, road[i].alpha_ground, g);
        std::copy(g.function.begin(), g.function.end(), batch.function.begin() + i * H);
        std::copy(g.normalization.begin(), g.normalization.end(), batch.normalization.begin() + i * H);
        std::copy(g.inv_sigma2.begin(), g.inv_sigma2.end(), batch.inv_sigma2.begin() + i * H);
    }
}

/* The host half of ComputeBatch / ComputeBatchGather: back to the fixed-stride layout incl. each column's
 * terminator -- what lies behind a terminator is unspecified, as in Compute().  A count is clamped to the
 * sections a column can hold before its terminator. */
void Stixels::ScatterSections(const int32_t* counts, const Section* packed, size_t total,
                              std::vector<StixelsData>& out) const {
    Section term;
    std::memset(&term, 0, sizeof(term));
    term.type = -1; /* StixelsKernels.cu:952-954 */
    size_t o = 0;
    for (size_t i = 0; i < out.size(); i++) {
        Section* dst = out[i].sections.data();
        for (int c = 0; c < m_realcols; c++) {
            int32_t n = counts[i * m_realcols + c];
            n = n < 0 ? 0 : (n > m_max_sections - 1 ? m_max_sections - 1 : n);
            if (o + (size_t)n > total) throw std::runtime_error("Stixels: the column counts exceed the packed sections.");
            if (n > 0) std::memcpy(dst + (size_t)c * m_max_sections, packed + o, (size_t)n * sizeof(Section));
            dst[(size_t)c * m_max_sections + n] = term;
            o += (size_t)n;
        }
    }
}

/* the packed payload of a batch (ComputeBatch, ComputeBatchGather): allocated on first use, released by Finish */
void Stixels::ReservePackBuffers() {
    const size_t cols = (size_t)m_max_batch * m_realcols;
    d_pack_counts.reserve(cols);
    d_pack_offsets.reserve(cols + 1);
    d_pack_sections.reserve(cols * (m_max_sections - 1));
    h_pack_offsets.reserve(cols + 1);
    h_pack_sections.reserve(cols * 64); /* (grown to what a batch needs by its caller) */
}

void Stixels::ComputeBatch(bool pairwise, int n_images, const pixel_t* d_big,
                           const int32_t* d_seg, const RoadParameters* road,
                           std::vector<StixelsData>& out, void* stream,
                           std::vector<InstanceMapping>* instance_stixels) {
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("n_images outside [1, max_batch] of InitializeBatch().");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    GroundModel g;
    std::vector<int> vh;
    BatchGround(n_images, road, g, vh);
    IS_CHECK_RETURN(is_join_columns(m_ctx, d_big, m_cols, m_median_join ? 1 : 0, d_disparity.get(),
                                    n_images, stream));
    /* instance candidates + clustering of every frame: two more launches for the whole batch */
    std::vector<is_instance_buffers> ibs;
    if (instance_stixels)
        for (int i = 0; i < n_images; i++) ibs.push_back(InstanceBuffers(i));
    IS_CHECK_RETURN(is_compute(m_ctx, d_disparity.get(), d_seg, g.function.data(), g.normalization.data(),
                               g.inv_sigma2.data(), vh.data(), pairwise ? 1 : 0, n_images, d_stixels,
                               instance_stixels ? ibs.data() : nullptr, nullptr, nullptr, stream));
    std::vector<float> alpha(n_images);
    for (int i = 0; i < n_images; i++) alpha[i] = road[i].alpha_ground;
    RememberBatch(n_images, instance_stixels != nullptr, alpha.data(), vh.data());
    DeliverBatch(n_images, road, false, out, stream, instance_stixels);
}

void Stixels::ComputeBatchRoad(bool pairwise, int n_images, const pixel_t* d_big, const int32_t* d_seg,
                               const RoadParameters* d_road, const uint8_t* d_status, std::vector<StixelsData>& out,
                               void* stream, std::vector<InstanceMapping>* instance_stixels,
                               std::vector<RoadParameters>* road_out, std::vector<uint8_t>* status_out) {
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("n_images outside [1, max_batch] of InitializeBatch().");
    if (!d_road || !d_status) throw std::invalid_argument("ComputeBatchRoad: null road parameters or status.");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    ForgetBatch(); /* (the road of this batch is known behind the synchronisation: DeliverBatch records it) */
    IS_CHECK_RETURN(is_join_columns(m_ctx, d_big, m_cols, m_median_join ? 1 : 0, d_disparity.get(),
                                    n_images, stream));
    std::vector<is_instance_buffers> ibs;
    if (instance_stixels)
        for (int i = 0; i < n_images; i++) ibs.push_back(InstanceBuffers(i));
    static_assert(sizeof(RoadParameters) == sizeof(is_road_params), "d_road holds is_road_params records");
    IS_CHECK_RETURN(is_compute_road(m_ctx, d_disparity.get(), d_seg, (const is_road_params*)d_road, pairwise ? 1 : 0,
                                    n_images, d_stixels, instance_stixels ? ibs.data() : nullptr, nullptr, nullptr,
                                    m_road_vhor_hint, stream));
    /* the road records and the status bytes: one small pinned block, in the queue of the pack offsets */
    RoadParameters* h_rp = (RoadParameters*)h_road.get();
    uint8_t* h_st = (uint8_t*)(h_rp + m_max_batch);
    IS_CHECK_RETURN(is_memcpy_d2h(h_rp, d_road, (size_t)n_images * sizeof(RoadParameters), stream));
    IS_CHECK_RETURN(is_memcpy_d2h(h_st, d_status, (size_t)n_images, stream));
    DeliverBatch(n_images, h_rp, true, out, stream, instance_stixels);
    /* the horizons of this batch plan the next one's launches (a road moves slowly from batch to batch; the hint
     * decides launch geometry only, never results) */
    m_road_vhor_hint = m_rows;
    for (int i = 0; i < n_images; i++) m_road_vhor_hint = std::min(m_road_vhor_hint, m_rows - h_rp[i].vhor - 1);
    m_road_vhor_hint = std::max(m_road_vhor_hint, 0);
    if (road_out) road_out->assign(h_rp, h_rp + n_images);
    if (status_out) status_out->assign(h_st, h_st + n_images);
}

void Stixels::DeliverBatch(int n_images, const RoadParameters* road, bool remember, std::vector<StixelsData>& out,
                           void* stream, std::vector<InstanceMapping>* instance_stixels) {
    /* Results to the host COMPACTED and through pinned memory: a column uses 10-60 of its 200 slots, and the
     * reference's fixed-stride copy (Stixels.cu:629-633: one frame) would move 1.6 MB per frame into pageable
     * vectors.  is_pack_sections leaves per-column offsets + the used sections; two pinned copies (the offsets, then
     * exactly the used sections) and a scatter on the host restore the fixed-stride layout. */
    const size_t ncols = (size_t)n_images * m_realcols;
    ReservePackBuffers();
    IS_CHECK_RETURN(is_pack_sections((const is_section*)d_stixels, (int)ncols, m_max_sections, d_pack_counts.get(),
                                     d_pack_offsets.get(), (is_section*)d_pack_sections.get(), stream));
    const int32_t* offsets = h_pack_offsets.get();
    IS_CHECK_RETURN(is_memcpy_d2h(h_pack_offsets.get(), d_pack_offsets.get(), (ncols + 1) * sizeof(int32_t), stream));
    if (instance_stixels) /* the per-class counts of all frames: one small copy */
        IS_CHECK_RETURN(is_memcpy_d2h(h_instance_head.get(), d_instances_per_class,
                                      (size_t)n_images * m_instance_classes * sizeof(int32_t), stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    std::vector<int> vh(n_images);
    for (int i = 0; i < n_images; i++) vh[i] = m_rows - road[i].vhor - 1;
    if (remember) {
        std::vector<float> alpha(n_images);
        for (int i = 0; i < n_images; i++) alpha[i] = road[i].alpha_ground;
        RememberBatch(n_images, instance_stixels != nullptr, alpha.data(), vh.data());
    }
    const size_t total = (size_t)offsets[ncols];
    m_last.known_offsets.resize(n_images + 1);
    for (int i = 0; i <= n_images; i++) m_last.known_offsets[i] = offsets[(size_t)i * m_realcols];
    if (total > h_pack_sections.capacity()) h_pack_sections.reserve(total + total / 4 + 1024);
    if (total > 0)
        IS_CHECK_RETURN(is_memcpy_d2h(h_pack_sections.get(), d_pack_sections.get(), total * sizeof(Section), stream));
    out.resize(n_images);
    for (int i = 0; i < n_images; i++) FillHeader(out[i], road[i].alpha_ground, vh[i]); /* (beside the copy) */
    std::vector<int32_t> counts(ncols);
    for (size_t col = 0; col < ncols; col++) counts[col] = offsets[col + 1] - offsets[col];
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    ScatterSections(counts.data(), h_pack_sections.get(), total, out);
    if (!instance_stixels) return;
    /* (column, section, label) triples of every frame, sized by the counts just read */
    const int32_t* head = h_instance_head.get();
    const size_t inst_n = (size_t)m_instance_classes * m_realcols * m_max_sections;
    std::vector<int> totals(n_images, 0);
    std::vector<std::vector<int32_t>> triples(n_images);
    for (int i = 0; i < n_images; i++) {
        for (int k = 0; k < m_instance_classes; k++) totals[i] += head[i * m_instance_classes + k];
        triples[i].resize(3 * (size_t)totals[i] + 1);
        if (totals[i] > 0)
            IS_CHECK_RETURN(is_memcpy_d2h(triples[i].data(), d_instance_packed.get() + (size_t)i * (1 + 3 * inst_n),
                                          (1 + 3 * (size_t)totals[i]) * sizeof(int32_t), stream));
    }
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    instance_stixels->assign(n_images, InstanceMapping());
    for (int i = 0; i < n_images; i++) {
        const int32_t* t = triples[i].data() + 1;
        for (int j = 0; j < totals[i]; j++)
            (*instance_stixels)[i][std::make_pair(t[3 * j], t[3 * j + 1])] = t[3 * j + 2];
    }
    /* a following GetInstanceStixels() returns the mapping of frame 0 (slice 0 of the arrays) */
    for (int k = 0; k < m_instance_classes; k++) m_instances_per_class[k] = head[k];
    m_labels_on_host = false;
}

/* ---------------------------------------------------------------- the last batch and its consumers */

void Stixels::RememberBatch(int frames, bool cluster_instances, const float* alpha, const int* vhor) {
    m_last.frames = frames;
    m_last.cluster_instances = cluster_instances;
    m_last.gt_instances = false;
    m_last.alpha.assign(alpha, alpha + frames);
    m_last.vhor.assign(vhor, vhor + frames);
    m_last.known_offsets.clear();
    m_sweep = Sweep(); /* (a sweep lasts until the next compute call; SweepBatch sets it behind this) */
}

void Stixels::ForgetBatch() { RememberBatch(0, false, nullptr, nullptr); }

struct Stixels::ConsumerScope { DeviceGuard guard; };

Stixels::ConsumerScope Stixels::BeginConsumer(const char* name, const char* verb, int n_images, void*& stream) {
    if (m_last.frames == 0)
        throw std::invalid_argument(std::string(name) + " " + verb +
                                    " the Sections of the last Compute() or ComputeBatch(): there are none.");
    if (n_images < 1 || n_images > m_last.frames)
        throw std::invalid_argument(std::string(name) + ": n_images outside [1, frames of the last compute call].");
    if (stream == nullptr) stream = m_stream;
    return ConsumerScope{DeviceGuard(m_ctx_device)};
}

template <class Args>
void Stixels::FillGeometry(Args& a, int n_images, int first) const {
    a.d_sections = (const is_section*)LastSections() + (size_t)first * m_realcols * m_max_sections;
    a.n_images = n_images;
    a.realcols = m_realcols;
    a.max_sections = m_max_sections;
    a.rows = m_rows;
    a.cols = m_cols;
}

void Stixels::FillGeometry(is_world_args& a, int n_images) const {
    a.d_sections = (const is_section*)LastSections();
    a.n_images = n_images;
    a.realcols = m_realcols;
    a.max_sections = m_max_sections;
    a.rows = m_rows;
}

void Stixels::CheckConsumer(const char* name, int rc) {
    if (rc == IS_EINVAL) throw std::invalid_argument(std::string(name) + ": " + is_last_error());
    IS_CHECK_RETURN(rc);
}

std::vector<Stixels::RenderResult> Stixels::RenderBatch(int n_images, const RenderTargets& t, void* stream) {
    const ConsumerScope scope = BeginConsumer("RenderBatch", "renders", n_images, stream);
    if (t.instance != nullptr && !HaveInstances())
        throw std::invalid_argument("RenderBatch: an instance image needs a compute call with instances.");
    const size_t B = (size_t)m_max_batch;
    const size_t res_bytes = B * (sizeof(double) + sizeof(int64_t) + sizeof(int32_t));
    d_render_results.reserve(res_bytes);
    h_render_results.reserve(res_bytes);
    double* d_sum = (double*)d_render_results.get();
    int64_t* d_cnt = (int64_t*)(d_render_results.get() + B * sizeof(double));
    int32_t* d_nst = (int32_t*)(d_render_results.get() + B * (sizeof(double) + sizeof(int64_t)));
    is_render_args a = {};
    FillGeometry(a, n_images);
    a.h_class_to_label = t.class_to_label;
    a.n_classes = t.n_classes;
    a.d_label = t.label;
    a.d_disparity = t.disparity;
    a.d_instance = t.instance;
    a.d_gt_label = t.gt_label;
    a.n_labels = t.n_labels;
    a.d_confusion = t.confusion;
    if (t.gt_disparity) {
        a.d_gt_disparity = t.gt_disparity;
        a.d_disp_abs_sum = d_sum;
        a.d_disp_count = d_cnt;
    } else {
        IS_CHECK_RETURN(is_memset(d_sum, 0, B * (sizeof(double) + sizeof(int64_t)), stream));
    }
    a.d_stixel_count = d_nst;
    if (t.instance) a.d_section_instance = SectionInstanceMap(n_images, stream);
    CheckConsumer("RenderBatch", is_render_sections(&a, stream));
    IS_CHECK_RETURN(is_memcpy_d2h(h_render_results.get(), d_render_results.get(), res_bytes, stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    const double* h_sum = (const double*)h_render_results.get();
    const int64_t* h_cnt = (const int64_t*)(h_render_results.get() + B * sizeof(double));
    const int32_t* h_nst = (const int32_t*)(h_render_results.get() + B * (sizeof(double) + sizeof(int64_t)));
    std::vector<RenderResult> out(n_images);
    for (int i = 0; i < n_images; i++) out[i] = RenderResult{h_sum[i], h_cnt[i], h_nst[i]};
    return out;
}

/* The map the three consumers read.  With the ground-truth map active nothing is launched. */
const int32_t* Stixels::SectionInstanceMap(int n_images, void* stream) {
    if (m_last.gt_instances) return d_section_instance_gt.get();
    if (!m_last.cluster_instances) return nullptr;
    d_section_instance.reserve((size_t)m_max_batch * m_realcols * m_max_sections);
    std::vector<is_instance_buffers> ibs;
    for (int i = 0; i < n_images; i++) ibs.push_back(LastInstanceBuffers(i));
    IS_CHECK_RETURN(is_section_instance_labels(ibs.data(), n_images, m_realcols, m_max_sections,
                                               d_section_instance.get(), stream));
    return d_section_instance.get();
}

/* Replaces the reference's --usegtoffsets producer (inference.py:388-396 over cityscapes.py:146-167) for a batch. */
void Stixels::GroundTruthOffsetsBatch(int n_images, const int32_t* d_gt, int32_t* d_seg, void* stream) {
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("GroundTruthOffsetsBatch: n_images outside [1, max_batch] of InitializeBatch().");
    if (d_gt == nullptr || d_seg == nullptr)
        throw std::invalid_argument("GroundTruthOffsetsBatch: null d_gt_instance or d_segmentation.");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    is_gt_targets_args a = {};
    a.d_gt_instance = d_gt;
    a.n_images = n_images;
    a.rows = m_rows;
    a.cols = m_cols;
    a.d_segmentation = d_seg;
    a.rows_power2_segmentation = m_params.rows_power2_segmentation;
    a.channels = m_segmentation_channels;
    a.scratch_bytes = is_gt_targets_scratch_bytes(m_max_batch, m_rows, m_cols, 0, 0);
    if (a.scratch_bytes == 0)
        throw std::invalid_argument("GroundTruthOffsetsBatch: rows and cols must be multiples of 8.");
    d_gt_targets_scratch.reserve(a.scratch_bytes);
    a.d_scratch = d_gt_targets_scratch.get();
    CheckConsumer("GroundTruthOffsetsBatch", is_gt_instance_targets(&a, stream));
}

/* The head of the reference's models (DRNDownsampled.py:97-102, :128-137) and its wrapper (wrappers.py:35-61). */
void Stixels::SetSegmentationHead(const std::vector<float>& weight, const std::vector<float>& bias, int K) {
    if (m_segmentation_channels < 1 || bias.size() != (size_t)m_segmentation_channels)
        throw std::invalid_argument("SetSegmentationHead: bias.size() is not the classes + instance channels of "
                                    "SetSegmentationParameters.");
    if (K < 8 || K % 8) throw std::invalid_argument("SetSegmentationHead: K must be >= 8 and a multiple of 8.");
    if (weight.size() != bias.size() * (size_t)K)
        throw std::invalid_argument("SetSegmentationHead: weight.size() is not bias.size() * K.");
    m_seghead_values.assign(weight.begin(), weight.end());
    m_seghead_values.insert(m_seghead_values.end(), bias.begin(), bias.end());
    m_seghead_K = K;
    m_seghead_uploaded = false;
}

void Stixels::SetSegmentationHeadClamp(int channel, float lo, float hi) {
    if (channel != -1 && !(lo <= hi)) throw std::invalid_argument("SetSegmentationHeadClamp: lo must be <= hi.");
    m_seghead_clamp_channel = channel;
    m_seghead_clamp_lo = lo;
    m_seghead_clamp_hi = hi;
}

void Stixels::SegmentationHeadBatch(int n_images, const void* d_features, int dtype, int32_t* d_seg, float* d_cnn_out,
                                    void* stream) {
    if (!m_is_initialized) throw std::invalid_argument("SegmentationHeadBatch: the object is not initialised.");
    if (m_seghead_K == 0 || m_seghead_values.size() != (size_t)m_segmentation_channels * (m_seghead_K + 1))
        throw std::invalid_argument("SegmentationHeadBatch: SetSegmentationHead() has not been called for the "
                                    "configured channels.");
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("SegmentationHeadBatch: n_images outside [1, max_batch] of InitializeBatch().");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    if (!m_seghead_uploaded || d_head_weights.get() == nullptr) {
        /* (on the object's stream and finished here: the caller's stream may be any other) */
        d_head_weights.reserve(m_seghead_values.size());
        IS_CHECK_RETURN(is_memcpy_h2d(d_head_weights.get(), m_seghead_values.data(), sizeof(float) * m_seghead_values.size(),
                                      m_stream));
        IS_CHECK_RETURN(is_stream_synchronize(m_stream));
        m_seghead_uploaded = true;
    }
    is_segmentation_head_args a = {};
    a.d_features = d_features;
    a.dtype = dtype;
    a.n_images = n_images;
    a.K = m_seghead_K;
    a.rows8 = m_rows / 8;
    a.cols8 = m_realcols;
    a.d_weight = d_head_weights.get();
    a.d_bias = d_head_weights.get() + (size_t)m_segmentation_channels * m_seghead_K;
    a.n_classes = m_segmentation_classes;
    a.n_regression = m_segmentation_channels - m_segmentation_classes;
    a.rows_power2_segmentation = m_params.rows_power2_segmentation;
    a.clamp_channel = m_seghead_clamp_channel;
    a.clamp_lo = m_seghead_clamp_lo;
    a.clamp_hi = m_seghead_clamp_hi;
    a.d_cnn_out = d_cnn_out;
    a.d_segmentation = d_seg;
    CheckConsumer("SegmentationHeadBatch", is_segmentation_head(&a, stream));
}

/* The CNN row of the reference's evaluation (tools/run_cityscapes.py:353-365, 551) from the head's float output. */
void Stixels::CnnLabelBatch(int n_images, const float* d_cnn_out, int mode, const CnnLabelTargets& t, void* stream) {
    if (!m_is_initialized) throw std::invalid_argument("CnnLabelBatch: the object is not initialised.");
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("CnnLabelBatch: n_images outside [1, max_batch] of InitializeBatch().");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    is_cnn_label_args a = {};
    a.d_cnn_out = d_cnn_out;
    a.n_images = n_images;
    a.channels = m_segmentation_channels;
    a.n_classes = m_segmentation_classes;
    a.rows8 = m_rows / 8;
    a.cols8 = m_realcols;
    a.mode = mode;
    a.rows = m_rows;
    a.cols = m_cols;
    a.d_class8 = t.class8;
    a.d_label = t.label;
    a.d_gt_label = t.gt_label;
    a.n_labels = t.n_labels;
    a.d_confusion = t.confusion;
    CheckConsumer("CnnLabelBatch", is_cnn_label_maps(&a, stream));
}

void Stixels::SetGTAssignmentParameters(double min_fraction, const int* label_ids8, bool gt_is_train_ids) {
    static const int kCityscapes[IS_INSTANCE_CLASSES] = {24, 25, 26, 27, 28, 31, 32, 33};
    if (min_fraction != min_fraction) throw std::invalid_argument("SetGTAssignmentParameters: min_fraction is NaN.");
    const int* ids = label_ids8 ? label_ids8 : kCityscapes;
    for (int i = 0; i < IS_INSTANCE_CLASSES; i++)
        if (ids[i] < 0 || ids[i] > 2147482)
            throw std::invalid_argument("SetGTAssignmentParameters: label id outside [0, 2147482].");
    m_gt_min_fraction = min_fraction;
    for (int i = 0; i < IS_INSTANCE_CLASSES; i++) m_gt_label_ids[i] = ids[i];
    m_gt_is_train_ids = gt_is_train_ids;
}

/* Replaces assign_instances_gt of the reference tooling (clustering_visualization.py:846-891) for a batch. */
void Stixels::AssignInstancesGTBatch(int n_images, const int32_t* d_gt, void* stream,
                                     std::vector<InstanceMapping>* mapping) {
    const ConsumerScope scope = BeginConsumer("AssignInstancesGTBatch", "labels", n_images, stream);
    if (d_gt == nullptr) throw std::invalid_argument("AssignInstancesGTBatch: null d_gt_instance.");
    const size_t cs = (size_t)m_realcols * m_max_sections;
    d_section_instance_gt.reserve((size_t)m_max_batch * cs);
    is_assign_gt_args a = {};
    FillGeometry(a, n_images);
    a.d_gt_instance = d_gt;
    /* (a 0 in the C struct selects its default; a negative fraction rejects exactly what 0 rejects: nothing) */
    a.min_fraction = m_gt_min_fraction == 0.0 ? -1.0 : m_gt_min_fraction;
    a.h_label_ids = m_gt_label_ids;
    a.gt_is_train_ids = m_gt_is_train_ids ? 1 : 0;
    a.d_section_instance = d_section_instance_gt.get();
    CheckConsumer("AssignInstancesGTBatch", is_assign_instances_gt(&a, stream));
    if (n_images < m_last.frames) /* the frames the vote did not cover have no instances */
        IS_CHECK_RETURN(is_memset(d_section_instance_gt.get() + n_images * cs, 0xff,
                                  (size_t)(m_last.frames - n_images) * cs * sizeof(int32_t), stream));
    m_last.gt_instances = true;
    if (!mapping) return;
    /* the labelled sections as quads behind their count: a label needs a section, so the sections of the batch
     * (counted by ComputeBatch; every slot in front of a terminator after a Compute()) bound the quads */
    const size_t cap = !m_last.known_offsets.empty() ? (size_t)m_last.known_offsets[n_images]
                                                     : (size_t)n_images * m_realcols * (m_max_sections - 1);
    const size_t words = 4 + 4 * cap;
    h_section_instance_gt.reserve(words);
    DeviceArray<int32_t>& d_packed = d_section_instance_gt_packed;
    d_packed.reserve(words);
    IS_CHECK_RETURN(is_pack_section_labels(d_section_instance_gt.get(), n_images, m_realcols, m_max_sections, (int)cap,
                                           d_packed.get(), stream));
    IS_CHECK_RETURN(is_memcpy_d2h(h_section_instance_gt.get(), d_packed.get(), words * sizeof(int32_t), stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    const int32_t* h = h_section_instance_gt.get();
    if ((size_t)h[0] > cap) throw std::runtime_error("AssignInstancesGTBatch: more labelled sections than sections.");
    mapping->assign(n_images, InstanceMapping());
    for (int j = 0; j < h[0]; j++) {
        const int32_t* q = h + 4 + 4 * (size_t)j;
        (*mapping)[q[0]][std::make_pair(q[1], q[2])] = q[3];
    }
}

void Stixels::SetInstanceOverlapCapacity(int records) {
    if (records < 1 || records > IS_OVERLAP_MAX_CAPACITY)
        throw std::invalid_argument("SetInstanceOverlapCapacity: records outside [1, IS_OVERLAP_MAX_CAPACITY].");
    m_overlap_capacity = records;
}

std::vector<std::vector<is_overlap_record>> Stixels::InstanceOverlapBatch(int n_images, const int32_t* d_gt,
                                                                          void* stream) {
    const ConsumerScope scope = BeginConsumer("InstanceOverlapBatch", "scores", n_images, stream);
    if (!HaveInstances())
        throw std::invalid_argument("InstanceOverlapBatch: needs a compute call with instances.");
    if (d_gt == nullptr) throw std::invalid_argument("InstanceOverlapBatch: null d_gt_instance.");
    const size_t B = (size_t)m_max_batch;
    const size_t cs = (size_t)m_realcols * m_max_sections;
    const size_t cap = (size_t)m_overlap_capacity;
    d_overlap_header.reserve(2 * B);
    h_overlap_header.reserve(2 * B);
    d_overlap_records.reserve(B * cap);
    d_overlap_packed.reserve(B * cap);
    h_overlap_packed.reserve(B * cap);
    const int32_t* const section_instance = SectionInstanceMap(n_images, stream);
    const size_t frame_px = (size_t)m_rows * m_cols;
    auto args = [&](int first, int n, int capacity, is_overlap_record* rec, int32_t* hdr) {
        is_instance_overlap_args a = {};
        FillGeometry(a, n, first);
        a.d_section_instance = section_instance + first * cs;
        a.d_gt_instance = d_gt + first * frame_px;
        a.capacity = capacity;
        a.d_records = rec;
        a.d_n_records = hdr;
        a.d_overflow = hdr + n;
        return a;
    };
    /* the batch: tables, packed on the device; the per-frame counts first, then the used records */
    const int32_t* header = h_overlap_header.get();
    const is_instance_overlap_args a = args(0, n_images, (int)cap, d_overlap_records.get(), d_overlap_header.get());
    CheckConsumer("InstanceOverlapBatch", is_instance_overlap(&a, stream));
    IS_CHECK_RETURN(is_pack_overlap_records(d_overlap_records.get(), d_overlap_header.get(), n_images, (int)cap,
                                            d_overlap_packed.get(), stream));
    IS_CHECK_RETURN(is_memcpy_d2h(h_overlap_header.get(), d_overlap_header.get(), 2 * n_images * sizeof(int32_t),
                                  stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    size_t total = 0;
    for (int i = 0; i < n_images; i++) total += (size_t)header[i];
    if (total)
        IS_CHECK_RETURN(is_memcpy_d2h(h_overlap_packed.get(), d_overlap_packed.get(),
                                      total * sizeof(is_overlap_record), stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    std::vector<std::vector<is_overlap_record>> out(n_images);
    std::vector<int> retry;
    const is_overlap_record* packed = h_overlap_packed.get();
    size_t off = 0;
    for (int i = 0; i < n_images; i++) {
        const int m = header[i];
        if (header[n_images + i]) retry.push_back(i);
        out[i].assign(packed + off, packed + off + m);
        off += (size_t)m;
    }
    /* frames with more distinct pairs than the capacity: alone, with 8x the table until it fits (rows*cols always
     * does: a frame has no more pairs than pixels) */
    for (const int f : retry) {
        size_t c = cap;
        for (;;) {
            c = std::min(c * 8, frame_px);
            struct Table { /* this attempt's table, freed on every way out of the attempt */
                DeviceArray<is_overlap_record> rec;
                DeviceArray<int32_t> hdr;
                ~Table() { rec.release(); hdr.release(); }
            } t;
            t.rec.reserve(c);
            t.hdr.reserve(2);
            const is_instance_overlap_args r = args(f, 1, (int)c, t.rec.get(), t.hdr.get());
            int32_t hdr[2] = {0, 0};
            IS_CHECK_RETURN(is_instance_overlap(&r, stream));
            IS_CHECK_RETURN(is_memcpy_d2h(hdr, t.hdr.get(), sizeof(hdr), stream));
            IS_CHECK_RETURN(is_stream_synchronize(stream));
            if (!hdr[1]) {
                out[f].resize((size_t)hdr[0]);
                if (hdr[0])
                    IS_CHECK_RETURN(is_memcpy_d2h(out[f].data(), t.rec.get(), (size_t)hdr[0] * sizeof(is_overlap_record),
                                                  stream));
                IS_CHECK_RETURN(is_stream_synchronize(stream));
                break;
            }
            if (c >= frame_px) throw std::runtime_error("InstanceOverlapBatch: a table of rows*cols records overflowed.");
        }
    }
    return out;
}

void Stixels::SetWorldCapacity(int records_per_frame) {
    if (records_per_frame < 0 || records_per_frame > m_realcols * (m_max_sections - 1))
        throw std::invalid_argument("SetWorldCapacity: records_per_frame outside [0, realcols * (max_sections - 1)].");
    m_world_capacity = records_per_frame;
}

Stixels::World Stixels::WorldBatch(int n_images, void* stream) {
    World w;
    WorldBatch(n_images, w, stream);
    return w;
}

void Stixels::WorldBatch(int n_images, World& w, void* stream) {
    const is_world_stixel* records = WorldBatchView(n_images, w.frame_offsets, stream);
    w.stixels.resize((size_t)w.frame_offsets[n_images]);
    CopyWorldRecords(w.stixels.data(), records, w.stixels.size());
}

void Stixels::CopyWorldRecords(is_world_stixel* dst, const is_world_stixel* src, size_t n) {
    const size_t per_thread = ((size_t)1 << 20) / sizeof(is_world_stixel) * 8; /* 8 MB of records */
    const size_t parts = std::min<size_t>(8, n / per_thread);
    if (parts < 2) {
        if (n) std::memcpy(dst, src, n * sizeof(is_world_stixel));
        return;
    }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < parts; t++) {
        const size_t lo = n * t / parts, hi = n * (t + 1) / parts;
        pool.emplace_back([=] { std::memcpy(dst + lo, src + lo, (hi - lo) * sizeof(is_world_stixel)); });
    }
    for (auto& t : pool) t.join();
}

const is_world_stixel* Stixels::WorldBatchView(int n_images, std::vector<int32_t>& frame_offsets, void* stream) {
    const ConsumerScope scope = BeginConsumer("WorldBatch", "exports", n_images, stream);
    if (m_camera_center_x == -1 || m_camera_center_y == -1)
        throw std::invalid_argument("Camera parameters are not set.");
    const size_t B = (size_t)m_max_batch;
    const size_t frame_max = (size_t)m_realcols * (m_max_sections - 1);
    d_world_counts.reserve(B * m_realcols);
    d_world_offsets.reserve(B * m_realcols + 1);
    d_world_totals.reserve(B);
    h_world_totals.reserve(B);
    /* the first pass: the exact size where the last call counted its sections, else a capacity per frame */
    const bool known = m_world_capacity == 0 && !m_last.known_offsets.empty();
    size_t cap = known ? (size_t)m_last.known_offsets[n_images]
                       : std::min((size_t)(m_world_capacity ? m_world_capacity : 4096), frame_max) * n_images;
    is_world_args a = {};
    FillGeometry(a, n_images);
    a.d_section_instance = SectionInstanceMap(n_images, stream);
    a.column_step = m_column_step;
    a.focal = m_focal;
    a.baseline = m_baseline;
    a.camera_center_x = m_camera_center_x;
    a.camera_center_y = m_camera_center_y;
    a.h_alpha_ground = m_last.alpha.data();
    a.h_vhor = m_last.vhor.data();
    a.d_counts = d_world_counts.get();
    a.d_offsets = d_world_offsets.get();
    a.d_frame_totals = d_world_totals.get();
    const int32_t* totals = h_world_totals.get();
    size_t total = 0;
    for (int pass = 0;; pass++) {
        d_world.reserve(cap);
        a.capacity = (int)cap;
        a.d_world = d_world.get();
        CheckConsumer("WorldBatch", is_stixel_world(&a, stream));
        IS_CHECK_RETURN(is_memcpy_d2h(h_world_totals.get(), d_world_totals.get(), n_images * sizeof(int32_t), stream));
        if (known && pass == 0 && cap > 0) { /* the records ride behind the totals: one synchronisation */
            h_world.reserve(cap);
            IS_CHECK_RETURN(is_memcpy_d2h(h_world.get(), d_world.get(), cap * sizeof(is_world_stixel), stream));
        }
        IS_CHECK_RETURN(is_stream_synchronize(stream));
        total = 0;
        for (int i = 0; i < n_images; i++) total += (size_t)totals[i];
        if (total <= cap) {
            if (!(known && pass == 0) && total > 0) {
                h_world.reserve(total + total / 4);
                IS_CHECK_RETURN(is_memcpy_d2h(h_world.get(), d_world.get(), total * sizeof(is_world_stixel), stream));
                IS_CHECK_RETURN(is_stream_synchronize(stream));
            }
            break;
        }
        if (pass > 0 || total > frame_max * n_images)
            throw std::runtime_error("WorldBatch: the batch holds more records than its columns can.");
        cap = total; /* overflow: again, with the true total */
    }
    frame_offsets.resize(n_images + 1);
    frame_offsets[0] = 0;
    for (int i = 0; i < n_images; i++) frame_offsets[i + 1] = frame_offsets[i] + totals[i];
    return h_world.get();
}

void Stixels::SetInstanceObjectCapacity(int objects_per_frame) {
    if (objects_per_frame < 1 || objects_per_frame > IS_INSTANCE_CLASSES * 1000)
        throw std::invalid_argument("SetInstanceObjectCapacity: objects_per_frame outside [1, 8000].");
    m_object_capacity = objects_per_frame;
}

void Stixels::InstanceObjectsBatch(int n_images, InstanceObjects& out, void* stream) {
    const InstanceObjectsView v = InstanceObjectsBatchView(n_images, stream);
    out.frame_objects.assign(v.frame_objects, v.frame_objects + n_images);
    out.frame_points.assign(v.frame_points, v.frame_points + n_images);
    out.objects.assign(v.objects, v.objects + v.n_objects);
    out.points.assign(v.points, v.points + v.n_points);
}

Stixels::InstanceObjectsView Stixels::InstanceObjectsBatchView(int n_images, void* stream) {
    const ConsumerScope scope = BeginConsumer("InstanceObjectsBatch", "reduces", n_images, stream);
    const size_t B = (size_t)m_max_batch;
    /* [2] totals | [B] frame objects | [B] frame points, padded to 16 bytes | objects | points */
    const size_t head = (sizeof(int32_t) * (2 + 2 * B) + 15) / 16 * 16;
    size_t want_objects = std::max(m_objects_cap, (size_t)m_object_capacity * n_images);
    size_t want_points = std::max(m_object_points_cap, 8 * (size_t)m_object_capacity * n_images);
    is_instance_objects_args a = {};
    FillGeometry(a, n_images);
    a.d_section_instance = SectionInstanceMap(n_images, stream);
    const int32_t* h = nullptr;
    for (int pass = 0;; pass++) {
        if (want_objects > m_objects_cap || want_points > m_object_points_cap || d_objects_block.get() == nullptr) {
            /* grow: both blocks into locals, the members and the capacities only after both exist */
            const size_t bytes = head + want_objects * sizeof(is_instance_object) + want_points * sizeof(is_contour_point);
            DeviceArray<char> d_new;
            PinnedArray<char> h_new;
            d_new.reserve(bytes);
            try {
                h_new.reserve(bytes);
            } catch (...) {
                d_new.release();
                throw;
            }
            d_objects_block = std::move(d_new); /* (a swap: the locals now hold the old blocks) */
            h_objects_block = std::move(h_new);
            d_new.release();
            h_new.release();
            m_objects_cap = want_objects;
            m_object_points_cap = want_points;
        }
        const size_t used = head + m_objects_cap * sizeof(is_instance_object);
        char* const d = d_objects_block.get();
        a.object_capacity = (int)std::min<size_t>(m_objects_cap, 0x7fffffff);
        a.point_capacity = (int)std::min<size_t>(m_object_points_cap, 0x7fffffff);
        a.d_totals = (int32_t*)d;
        a.d_frame_objects = a.d_totals + 2;
        a.d_frame_points = a.d_frame_objects + B;
        a.d_objects = (is_instance_object*)(d + head);
        a.d_points = (is_contour_point*)(d + used);
        CheckConsumer("InstanceObjectsBatch", is_instance_objects(&a, stream));
        /* everything behind one synchronisation: the block is small (64 + 8 * 32 bytes per object of capacity) */
        IS_CHECK_RETURN(is_memcpy_d2h(h_objects_block.get(), d, used + m_object_points_cap * sizeof(is_contour_point),
                                      stream));
        IS_CHECK_RETURN(is_stream_synchronize(stream));
        h = (const int32_t*)h_objects_block.get();
        if ((size_t)h[0] <= m_objects_cap && (size_t)h[1] <= m_object_points_cap) break;
        if (pass > 0) throw std::runtime_error("InstanceObjectsBatch: the totals changed between two passes.");
        want_objects = std::max(m_objects_cap, (size_t)h[0]); /* overflow: again, with the true totals */
        want_points = std::max(m_object_points_cap, (size_t)h[1]);
    }
    InstanceObjectsView v;
    v.frame_objects = h + 2;
    v.frame_points = h + 2 + B;
    v.objects = (const is_instance_object*)(h_objects_block.get() + head);
    v.points = (const is_contour_point*)(h_objects_block.get() + head + m_objects_cap * sizeof(is_instance_object));
    v.n_objects = h[0];
    v.n_points = h[1];
    return v;
}

/* ---------------------------------------------------------------- parameter sweeps */

is_sweep_set Stixels::CoreSweepSet(const SweepSet& set) {
    is_sweep_set s = {};
    s.prior_weight = set.prior_weight;
    s.disparity_weight = set.disparity_weight;
    s.segmentation_weight = set.segmentation_weight;
    /* SetWeightParameters: the instance weight is expressed relative to the segmentation weight */
    s.instance_weight = 0.0;
    if (set.segmentation_weight > 1e-5) {
        s.instance_weight = set.instance_weight / set.segmentation_weight;
        if (set.instance_weight < 1e-8) s.instance_weight = 0.0;
    }
    s.clustering_eps = set.eps;
    s.clustering_min_pts = set.min_pts;
    s.clustering_size_filter = set.size_filter;
    return s;
}

/* One frame of d_sweep_instances, every part 16-byte aligned:
 * [8] per-class counts | centres [inst_n][2] | indices [inst_n][2] | labels [inst_n] | packed [1 + 3 inst_n] | core flags */
namespace {
struct SweepFrameLayout {
    size_t com, idx, labels, packed, core, stride;
    explicit SweepFrameLayout(size_t inst_n) {
        auto up = [](size_t b) { return (b + 15) / 16 * 16; };
        com = up(IS_INSTANCE_CLASSES * sizeof(int32_t));
        idx = com + up(inst_n * 2 * sizeof(float));
        labels = idx + up(inst_n * 2 * sizeof(int32_t));
        packed = labels + up(inst_n * sizeof(int32_t));
        core = packed + up((1 + 3 * inst_n) * sizeof(int32_t));
        stride = core + up(inst_n);
    }
};
}  // namespace

size_t Stixels::SweepInstanceStride() const {
    return SweepFrameLayout((size_t)m_instance_classes * m_realcols * m_max_sections).stride;
}

is_instance_buffers Stixels::SweepInstanceBuffers(int set, int image) const {
    const SweepFrameLayout l((size_t)m_instance_classes * m_realcols * m_max_sections);
    char* const f = d_sweep_instances.get() + ((size_t)set * m_sweep.frames + image) * l.stride;
    is_instance_buffers ib = {};
    ib.d_instances_per_class = (int32_t*)f;
    ib.d_centerofmass = (float*)(f + l.com);
    ib.d_indices = (int32_t*)(f + l.idx);
    ib.d_labels = (int32_t*)(f + l.labels);
    ib.d_packed = (int32_t*)(f + l.packed);
    ib.d_core_candidates = (uint8_t*)(f + l.core);
    return ib;
}

const Section* Stixels::LastSections() const {
    if (m_sweep.sets == 0) return d_stixels;
    return d_sweep_stixels.get() + (size_t)m_sweep.selected * m_sweep.frames * m_realcols * m_max_sections;
}

void Stixels::SweepBatch(bool pairwise, int n_images, const pixel_t* d_big, const int32_t* d_seg,
                         const RoadParameters* road, const std::vector<SweepSet>& sets, void* stream,
                         bool with_instances) {
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("n_images outside [1, max_batch] of InitializeBatch().");
    if (sets.empty()) throw std::invalid_argument("SweepBatch: no parameter sets.");
    const size_t cs = (size_t)m_realcols * m_max_sections;
    const size_t frames = sets.size() * (size_t)n_images;
    if (frames * cs > 0x7fffffffull)
        throw std::invalid_argument("SweepBatch: sets * n_images * realcols * max_sections does not fit 31 bits.");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    ForgetBatch(); /* (a sweep that fails leaves nothing to consume) */
    /* grow: only the array that is too small, into a local; the members after both exist */
    const size_t want_inst = with_instances ? frames * SweepInstanceStride() : 0;
    {
        DeviceArray<Section> s_new;
        DeviceArray<char> i_new;
        const bool grow_s = frames * cs > d_sweep_stixels.capacity(), grow_i = want_inst > d_sweep_instances.capacity();
        if (grow_s) s_new.reserve(frames * cs);
        try {
            if (grow_i) i_new.reserve(want_inst);
        } catch (...) {
            s_new.release();
            throw;
        }
        if (grow_s) d_sweep_stixels = std::move(s_new); /* (a swap: the local now holds the old array) */
        if (grow_i) d_sweep_instances = std::move(i_new);
        s_new.release();
        i_new.release();
    }
    GroundModel g;
    std::vector<int> vh;
    BatchGround(n_images, road, g, vh);
    IS_CHECK_RETURN(is_join_columns(m_ctx, d_big, m_cols, m_median_join ? 1 : 0, d_disparity.get(), n_images, stream));
    std::vector<is_sweep_set> core_sets;
    for (const SweepSet& set : sets) core_sets.push_back(CoreSweepSet(set));
    std::vector<float> alpha(n_images);
    for (int i = 0; i < n_images; i++) alpha[i] = road[i].alpha_ground;
    m_sweep.frames = n_images; /* (SweepInstanceBuffers: set k's frames lie behind k * frames frames) */
    std::vector<is_instance_buffers> ibs;
    if (with_instances)
        for (size_t k = 0; k < sets.size(); k++)
            for (int i = 0; i < n_images; i++) ibs.push_back(SweepInstanceBuffers((int)k, i));
    CheckConsumer("SweepBatch", is_compute_sweep(m_ctx, d_disparity.get(), d_seg, g.function.data(),
                                                 g.normalization.data(), g.inv_sigma2.data(), vh.data(), pairwise ? 1 : 0,
                                                 n_images, core_sets.data(), (int)core_sets.size(),
                                                 (is_section*)d_sweep_stixels.get(), with_instances ? ibs.data() : nullptr,
                                                 stream));
    RememberBatch(n_images, with_instances, alpha.data(), vh.data());
    m_sweep.sets = (int)sets.size();
    m_sweep.frames = n_images;
    m_sweep.selected = 0;
    m_sweep.instances = with_instances;
}

void Stixels::SelectSweepSet(int k) {
    if (m_sweep.sets == 0) throw std::invalid_argument("SelectSweepSet: the last compute call was not a SweepBatch().");
    if (k < 0 || k >= m_sweep.sets) throw std::invalid_argument("SelectSweepSet: k outside the sets of the last SweepBatch().");
    m_sweep.selected = k;
    m_last.cluster_instances = m_sweep.instances;
    m_last.gt_instances = false;
    m_last.known_offsets.clear();
}

void Stixels::FetchSections(const Section* d_sections, int n_images, const float* alpha, const int* vhor,
                            std::vector<StixelsData>& out, void* stream) {
    const size_t ncols = (size_t)n_images * m_realcols;
    ReservePackBuffers();
    IS_CHECK_RETURN(is_pack_sections((const is_section*)d_sections, (int)ncols, m_max_sections, d_pack_counts.get(),
                                     d_pack_offsets.get(), (is_section*)d_pack_sections.get(), stream));
    const int32_t* offsets = h_pack_offsets.get();
    IS_CHECK_RETURN(is_memcpy_d2h(h_pack_offsets.get(), d_pack_offsets.get(), (ncols + 1) * sizeof(int32_t), stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    const size_t total = (size_t)offsets[ncols];
    if (total > h_pack_sections.capacity()) h_pack_sections.reserve(total + total / 4 + 1024);
    if (total > 0)
        IS_CHECK_RETURN(is_memcpy_d2h(h_pack_sections.get(), d_pack_sections.get(), total * sizeof(Section), stream));
    out.resize(n_images);
    for (int i = 0; i < n_images; i++) FillHeader(out[i], alpha[i], vhor[i]);
    std::vector<int32_t> counts(ncols);
    for (size_t col = 0; col < ncols; col++) counts[col] = offsets[col + 1] - offsets[col];
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    ScatterSections(counts.data(), h_pack_sections.get(), total, out);
}

void Stixels::FetchInstanceMappings(const std::vector<is_instance_buffers>& ibs, std::vector<InstanceMapping>& out,
                                    void* stream) {
    const size_t n = ibs.size();
    const size_t slots = (size_t)m_instance_classes * m_realcols * m_max_sections;
    std::vector<int32_t> head(n * m_instance_classes);
    for (size_t i = 0; i < n; i++)
        IS_CHECK_RETURN(is_memcpy_d2h(head.data() + i * m_instance_classes, ibs[i].d_instances_per_class,
                                      m_instance_classes * sizeof(int32_t), stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    std::vector<size_t> totals(n, 0);
    std::vector<std::vector<int32_t>> triples(n);
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < m_instance_classes; k++)
            totals[i] += (size_t)std::min<int64_t>(std::max<int32_t>(head[i * m_instance_classes + k], 0),
                                                   (int64_t)m_realcols * m_max_sections);
        totals[i] = std::min(totals[i], slots);
        triples[i].resize(3 * totals[i] + 1);
        if (totals[i] > 0)
            IS_CHECK_RETURN(is_memcpy_d2h(triples[i].data(), ibs[i].d_packed, (1 + 3 * totals[i]) * sizeof(int32_t),
                                          stream));
    }
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    out.assign(n, InstanceMapping());
    for (size_t i = 0; i < n; i++) {
        const int32_t* t = triples[i].data() + 1;
        for (size_t j = 0; j < totals[i]; j++) out[i][std::make_pair(t[3 * j], t[3 * j + 1])] = t[3 * j + 2];
    }
}

void Stixels::SweepSections(int k, std::vector<StixelsData>& out, std::vector<InstanceMapping>* instance_stixels) {
    if (m_sweep.sets == 0) throw std::invalid_argument("SweepSections: the last compute call was not a SweepBatch().");
    if (k < 0 || k >= m_sweep.sets) throw std::invalid_argument("SweepSections: k outside the sets of the last SweepBatch().");
    if (instance_stixels && !m_sweep.instances)
        throw std::invalid_argument("SweepSections: the mappings need a SweepBatch() with instances.");
    const DeviceGuard guard(m_ctx_device);
    const int n = m_last.frames;
    FetchSections(d_sweep_stixels.get() + (size_t)k * n * m_realcols * m_max_sections, n, m_last.alpha.data(),
                  m_last.vhor.data(), out, m_stream);
    if (!instance_stixels) return;
    std::vector<is_instance_buffers> ibs;
    for (int i = 0; i < n; i++) ibs.push_back(SweepInstanceBuffers(k, i));
    FetchInstanceMappings(ibs, *instance_stixels, m_stream);
}

void Stixels::ReclusterBatch(float eps, int min_pts, int size_filter, std::vector<InstanceMapping>* instance_stixels,
                             void* stream) {
    if (m_last.frames == 0)
        throw std::invalid_argument("ReclusterBatch clusters the candidates of the last compute call: there are none.");
    if (!m_last.cluster_instances)
        throw std::invalid_argument("ReclusterBatch: needs a compute call with instances.");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    std::vector<is_instance_buffers> ibs;
    for (int i = 0; i < m_last.frames; i++) ibs.push_back(LastInstanceBuffers(i));
    CheckConsumer("ReclusterBatch", is_recluster(m_ctx, (const is_section*)LastSections(), m_last.frames, eps, min_pts,
                                                 size_filter, ibs.data(), stream));
    m_last.gt_instances = false; /* (as UseClusterInstances) */
    m_labels_on_host = false;
    if (instance_stixels) FetchInstanceMappings(ibs, *instance_stixels, stream);
}

void Stixels::SetInstanceDisparityCapacity(int keys_per_frame) {
    if (keys_per_frame < 1 || keys_per_frame > IS_INSTANCE_DISPARITY_KEYS)
        throw std::invalid_argument("SetInstanceDisparityCapacity: keys_per_frame outside [1, IS_INSTANCE_DISPARITY_KEYS].");
    m_idisp_capacity = keys_per_frame;
}

/* Replaces --use-disparity from_gt of the reference tooling (clustering_visualization.py:794-819, 894-960, 996-1049)
 * for a batch. */
void Stixels::ClusterInstanceDisparityBatch(int n_images, const int32_t* gt_instance, const uint8_t* disparity_u8,
                                            float eps, int min_pts, int size_filter,
                                            std::vector<InstanceMapping>* instance_stixels, float* stixel_median,
                                            void* stream, bool inputs_on_host) {
    const ConsumerScope scope = BeginConsumer("ClusterInstanceDisparityBatch", "clusters", n_images, stream);
    if (!m_last.cluster_instances)
        throw std::invalid_argument("ClusterInstanceDisparityBatch: needs a compute call with instances.");
    if (gt_instance == nullptr || disparity_u8 == nullptr)
        throw std::invalid_argument("ClusterInstanceDisparityBatch: null gt_instance or disparity_u8.");
    const size_t cs = (size_t)m_realcols * m_max_sections, px = (size_t)n_images * m_rows * m_cols;
    if (inputs_on_host) { /* gt | disparity, each 16-byte aligned */
        const size_t gt_bytes = (px * sizeof(int32_t) + 15) & ~(size_t)15;
        d_idisp_inputs.reserve(gt_bytes + px);
        IS_CHECK_RETURN(is_memcpy_h2d(d_idisp_inputs.get(), gt_instance, px * sizeof(int32_t), stream));
        IS_CHECK_RETURN(is_memcpy_h2d(d_idisp_inputs.get() + gt_bytes, disparity_u8, px, stream));
        IS_CHECK_RETURN(is_stream_synchronize(stream)); /* (the caller's arrays are free again on every way out) */
        gt_instance = (const int32_t*)d_idisp_inputs.get();
        disparity_u8 = (const uint8_t*)(d_idisp_inputs.get() + gt_bytes);
    }
    std::vector<is_instance_buffers> ibs;
    for (int i = 0; i < n_images; i++) ibs.push_back(LastInstanceBuffers(i));
    const size_t counts_bytes = ((size_t)m_max_batch * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t out_bytes = counts_bytes + (stixel_median ? (size_t)n_images * cs * sizeof(float) : 0);
    d_idisp_out.reserve(out_bytes);
    h_idisp_out.reserve(out_bytes);
    is_instance_disparity_args a = {};
    FillGeometry(a, n_images);
    a.d_gt_instance = gt_instance;
    a.d_disparity_u8 = disparity_u8;
    a.instances = ibs.data();
    a.eps = eps;
    a.min_pts = min_pts;
    a.size_filter = size_filter;
    a.capacity = m_idisp_capacity;
    a.scratch_bytes = is_instance_disparity_scratch_bytes(n_images, m_realcols, m_max_sections, m_idisp_capacity);
    d_idisp_scratch.reserve(std::max<size_t>(a.scratch_bytes, 16));
    a.d_scratch = d_idisp_scratch.get();
    a.d_key_count = (int32_t*)d_idisp_out.get();
    if (stixel_median) a.d_stixel_median = (float*)(d_idisp_out.get() + counts_bytes);
    CheckConsumer("ClusterInstanceDisparityBatch", is_cluster_instance_disparity(&a, stream));
    IS_CHECK_RETURN(is_memcpy_d2h(h_idisp_out.get(), d_idisp_out.get(), out_bytes, stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    const int32_t* keys = (const int32_t*)h_idisp_out.get();
    for (int i = 0; i < n_images; i++)
        if (keys[i] > m_idisp_capacity)
            throw std::runtime_error("ClusterInstanceDisparityBatch: frame " + std::to_string(i) + " holds " +
                                     std::to_string(keys[i]) + " ground-truth instances, the capacity is " +
                                     std::to_string(m_idisp_capacity) +
                                     " (SetInstanceDisparityCapacity); no label was changed.");
    if (stixel_median) std::memcpy(stixel_median, h_idisp_out.get() + counts_bytes, (size_t)n_images * cs * sizeof(float));
    m_last.gt_instances = false; /* (as ReclusterBatch) */
    m_labels_on_host = false;
    if (instance_stixels) FetchInstanceMappings(ibs, *instance_stixels, stream);
}

/* The shard of this rank, then the compacted gather of every rank's Sections on `dst` (the
 * C ABI underneath: is_pack_sections -> is_gather_sections -> is_unpack_sections). */
void Stixels::ComputeBatchGather(bool pairwise, int n_images, const pixel_t* d_big, const int32_t* d_seg,
                                 const RoadParameters* road, void* comm, int dst, const int* images_per_rank,
                                 const RoadParameters* road_all, std::vector<StixelsData>& out, void* stream) {
    if (n_images < 1 || n_images > m_max_batch)
        throw std::invalid_argument("n_images outside [1, max_batch] of InitializeBatch().");
    if (comm == nullptr || images_per_rank == nullptr)
        throw std::invalid_argument("ComputeBatchGather needs a communicator and the shard sizes.");
    const DeviceGuard guard(m_ctx_device);
    if (stream == nullptr) stream = m_stream;
    int rank = 0, nranks = 0;
    IS_CHECK_RETURN(is_comm_rank(comm, &rank, &nranks));
    if (images_per_rank[rank] != n_images)
        throw std::invalid_argument("images_per_rank[rank] differs from n_images.");
    if (rank == dst && road_all == nullptr)
        throw std::invalid_argument("the destination rank needs road_all (the headers of every frame).");
    const int my_cols = n_images * m_realcols;

    /* ---- this rank's shard: ground model on the host, JoinColumns + DP + back-trace on the device */
    GroundModel g;
    std::vector<int> vh;
    BatchGround(n_images, road, g, vh);
    IS_CHECK_RETURN(is_join_columns(m_ctx, d_big, m_cols, m_median_join ? 1 : 0, d_disparity.get(), n_images,
                                    stream));
    IS_CHECK_RETURN(is_compute(m_ctx, d_disparity.get(), d_seg, g.function.data(), g.normalization.data(),
                               g.inv_sigma2.data(), vh.data(), pairwise ? 1 : 0, n_images, d_stixels, nullptr,
                               nullptr, nullptr, stream));
    ForgetBatch(); /* (d_stixels now holds this rank's shard; the consumers read Compute / ComputeBatch) */

    /* ---- pack: per-column counts + the used sections (10-40 of the 200 slots of a column) */
    ReservePackBuffers();
    IS_CHECK_RETURN(is_pack_sections((const is_section*)d_stixels, my_cols, m_max_sections, d_pack_counts.get(),
                                     d_pack_offsets.get(), (is_section*)d_pack_sections.get(), stream));

    /* ---- gather on dst.  Landing buffers: counts for every column, sections for 64 per column at first
     * (synthetic and real scenes use 10-60); when a batch needs more, EVERY rank sees IS_ENOMEM from the
     * gather (dst's go-ahead), dst grows to the worst case and all ranks repeat the call.  A landing buffer
     * is replaced only after the stream has finished with the old one. */
    std::vector<int32_t> columns(nranks);
    size_t all_cols = 0;
    int all_images = 0;
    for (int r = 0; r < nranks; r++) {
        columns[r] = images_per_rank[r] * m_realcols;
        all_cols += (size_t)columns[r];
        all_images += images_per_rank[r];
    }
    std::vector<int64_t> totals(nranks, 0);
    if (rank == dst && d_all_counts.capacity() < (all_cols + 1) * 2) {
        IS_CHECK_RETURN(is_stream_synchronize(stream));
        d_all_counts.reserve((all_cols + 1) * 2);
    }
    for (int attempt = 0;; attempt++) {
        if (rank == dst) {
            const size_t want = attempt == 0 ? all_cols * 64 : all_cols * (size_t)(m_max_sections - 1);
            if (d_all_packed.capacity() < want) {
                IS_CHECK_RETURN(is_stream_synchronize(stream));
                d_all_packed.reserve(want);
            }
        }
        const int rc = is_gather_sections(comm, dst, columns.data(), d_pack_counts.get(), d_pack_offsets.get(),
                                          (const is_section*)d_pack_sections.get(), d_all_counts.get(),
                                          (is_section*)d_all_packed.get(), d_all_packed.capacity(), totals.data(),
                                          stream);
        if (rc == IS_ENOMEM && attempt == 0) continue; /* (every rank takes this branch together) */
        IS_CHECK_RETURN(rc);
        break;
    }
    out.clear();
    if (rank != dst) {
        IS_CHECK_RETURN(is_stream_synchronize(stream)); /* the payload has left before the buffers are reused */
        return;
    }
    /* ---- dst: the packed payload of all ranks to the host through pinned memory (per-column counts + exactly the used
     * sections), then back to fixed-stride Section arrays on the host -- like ComputeBatch; is_unpack_sections is the
     * device-side form of the same scatter for callers that keep the result on the GPU */
    size_t total = 0;
    for (int r = 0; r < nranks; r++) total += (size_t)totals[r];
    h_all_counts.reserve(all_cols);
    if (total > h_pack_sections.capacity()) h_pack_sections.reserve(total + total / 4 + 1024);
    IS_CHECK_RETURN(is_memcpy_d2h(h_all_counts.get(), d_all_counts.get(), all_cols * sizeof(int32_t), stream));
    if (total > 0)
        IS_CHECK_RETURN(is_memcpy_d2h(h_pack_sections.get(), d_all_packed.get(), total * sizeof(Section), stream));
    out.resize(all_images);
    for (int i = 0; i < all_images; i++) FillHeader(out[i], road_all[i].alpha_ground, m_rows - road_all[i].vhor - 1);
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    ScatterSections(h_all_counts.get(), h_pack_sections.get(), total, out);
}

/* ---------------------------------------------------------------- instances */

/* Size-filtered DBSCAN over the predicted instance centres of each instance class, on the
 * device (k_cluster_instances, csrc/is_k_cluster.hip).  The reference calls a cuML fork whose
 * source is not in its tree (Stixels.cu:639-681); the semantics are those of
 * its Python twin (/root/reference/tools/visualization/clustering_visualization.py:894-960).
 * Compute() already runs it; calling it again re-clusters the candidates of the last frame with
 * the eps / min_pts of Initialize() (m_params, like the reference). */
float Stixels::ClusterInstances() {
    const DeviceGuard guard(m_ctx_device);
    const is_instance_buffers ib = InstanceBuffers();
    IS_CHECK_RETURN(is_cluster_instances(m_ctx, &ib, m_stream));
    m_labels_on_host = false;
    return -1;
}

std::map<std::pair<int, int>, int> Stixels::GetInstanceStixels() { /* Stixels.cu:744-776 */
    /* the reference copies the complete label and index arrays (4.8 MB, "~0.8 milliseconds",
     * :745); here the device has packed (column, section, label) triples of the candidates */
    if (!m_labels_on_host) {
        const DeviceGuard guard(m_ctx_device);
        int total = 0;
        for (int k = 0; k < m_instance_classes; k++) total += m_instances_per_class[k];
        if (total > 0) {
            IS_CHECK_RETURN(is_memcpy_d2h(h_instance_packed.get(), d_instance_packed.get(),
                                          (1 + 3 * (size_t)total) * sizeof(int32_t), m_stream));
            IS_CHECK_RETURN(is_stream_synchronize(m_stream));
        } else {
            h_instance_packed.get()[0] = 0;
        }
        m_labels_on_host = true;
    }
    std::map<std::pair<int, int>, int> mapping;
    const int total = h_instance_packed.get()[0];
    const int32_t* t = h_instance_packed.get() + 1;
    for (int i = 0; i < total; i++)
        mapping[std::make_pair(t[3 * i], t[3 * i + 1])] = t[3 * i + 2];
    return mapping;
}

/* ---------------------------------------------------------------- outputs */

std::vector<float> Stixels::Get3DVertices(const StixelsData& stixels_data) { /* :683-742 */
    if (m_camera_center_x == -1 || m_camera_center_y == -1)
        throw std::invalid_argument("Camera parameters are not set.");
    std::vector<float> vertices;
    for (size_t i = 0; i < (size_t)m_realcols; i++) {
        for (size_t j = 0; j < (size_t)m_max_sections; j++) {
            const Section& section = stixels_data.sections[i * m_max_sections + j];
            if (section.type == -1) break;
            const float x_l = i * m_column_step;
            const float x_r = x_l + m_column_step;
            const float y_t = m_rows - section.vT - 1;
            const float y_b = m_rows - section.vB;
            float top_depth = 0.0, bottom_depth = 0.0; /* sky stays at depth 0 */
            if (section.type == OBJECT) {
                top_depth = m_baseline * m_focal / section.disparity;
                bottom_depth = top_depth;
            } else if (section.type == GROUND) {
                const float top_disparity =
                    stixels_data.alpha_ground * (stixels_data.vhor - section.vT);
                const float bottom_disparity =
                    stixels_data.alpha_ground * (stixels_data.vhor - section.vB);
                top_depth = m_baseline * m_focal / top_disparity;
                bottom_depth = m_baseline * m_focal / bottom_disparity;
            }
            const float corner[4][3] = {
                {x_l, y_t, top_depth}, {x_r, y_t, top_depth},
                {x_r, y_b, bottom_depth}, {x_l, y_b, bottom_depth}}; /* clockwise from top left */
            for (const auto& c : corner) {
                vertices.push_back(-c[2] / m_focal * (m_camera_center_x - c[0]));
                vertices.push_back(-c[2] / m_focal * (m_camera_center_y - c[1]));
                vertices.push_back(c[2]);
            }
        }
    }
    return vertices;
}

void Stixels::SaveStixels(Section* stixels,
                          std::map<std::pair<int, int>, int> instance_stixels_mapping,
                          const float alpha_ground, const int vhor, const int real_cols,
                          const int max_segments, const char* fname) { /* Stixels.cu:889-926 */
    std::ofstream fp;
    fp.open(fname, std::ofstream::out | std::ofstream::trunc);
    if (!fp.is_open()) {
        std::cerr << "Counldn't write file: " << fname << std::endl;
        return;
    }
    for (size_t i = 0; i < (size_t)real_cols; i++) {
        for (size_t j = 0; j < (size_t)max_segments; j++) {
            const Section& section = stixels[i * max_segments + j];
            if (section.type == -1) break;
            fp << section.type << "," << section.vB << "," << section.vT << ","
               << section.disparity << "," << section.semantic_class << "," << section.cost << ","
               << section.instance_meanx << "," << section.instance_meany;
            const auto it = instance_stixels_mapping.find(std::make_pair((int)i, (int)j));
            if (it != instance_stixels_mapping.end()) fp << "," << (*it).second;
            fp << ";";
        }
        fp << std::endl;
    }
    fp << "groundplane" << alpha_ground << "," << vhor << "\n";
    fp.close();
}
