/*
 * RoadEstimation.cpp -- host class of the road estimation step, the
 * producer of the four scalars Stixels::SetRoadParameters consumes.  Mirrors
 * /root/reference/InstanceStixels/src/RoadEstimation.cu:32-193; citations `RE.cu:N` refer to it.
 * Device work goes through the C ABI (is_road_vdisparity); the line fit runs on the host like
 * the reference's cv::HoughLines call, with an own implementation of the standard transform.
 */
#include "InstanceStixels/RoadEstimation.h"
#include "DeviceGuard.h"
#include "is_ground_model.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>

static const float kPi = 3.1415926535897932384626433832795f; /* CV_PI as float */

RoadEstimation::RoadEstimation() {}
RoadEstimation::~RoadEstimation() {}

void RoadEstimation::Initialize(const float camera_center_y, const float baseline,
                                const float focal, const int rows, const int cols,
                                const int max_dis, const float road_vdisparity_threshold) {
    /* re-initialisation (a new frame shape or camera, stixels_wrapper.cu:124-152) releases the stream and the
     * buffers of the previous one first -- on THEIR device, which Finish() still knows */
    if (m_is_initialized || m_stream) Finish();
    SetCamera(camera_center_y, baseline, focal, rows);
    m_HoughAccumThr = 25; /* RE.cu:45-57 */
    m_binThr = road_vdisparity_threshold;
    m_maxCameraHeight = 1.90f;
    m_minCameraHeight = 1.30f;
    m_max_dis = max_dis;
    m_cols = cols;
    m_rho = m_theta = 0;
    m_horizonPoint = 0;
    m_pitch = m_cameraHeight = 0;
    m_vDisp.assign((size_t)m_max_dis * m_rows, 0);
    /* the device of the buffers: SetDevice(), else the caller's current one (like Stixels::Initialize) */
    int device = m_device;
    if (device < 0) IS_CHECK_RETURN(is_get_device(&device));
    m_ctx_device = device;
    const DeviceGuard guard(device);
    IS_CHECK_RETURN(is_stream_create(&m_stream, 1));
    d_disparity.reserve((size_t)m_cols * m_rows);
    d_vDisp.reserve((size_t)m_max_dis * m_rows);
    d_maximum.reserve(1);
    d_vDispBinary.reserve((size_t)m_max_dis * m_rows);
    m_is_initialized = true;
}

void RoadEstimation::SetCamera(float camera_center_y, float baseline, float focal, int rows) {
    m_cy = camera_center_y; /* RE.cu:37-40 */
    m_b = baseline;
    m_focal = focal;
    PitchGate(m_minPitch, m_maxPitch);
    m_rows = rows;
}

void RoadEstimation::Finish() { /* RE.cu:84-92 */
    const DeviceGuard guard(m_ctx_device);
    if (m_stream) {
        IS_CHECK_RETURN(is_stream_synchronize(m_stream));
        IS_CHECK_RETURN(is_stream_destroy(m_stream));
        m_stream = nullptr;
    }
    d_vDisp.release();
    d_disparity.release();
    d_maximum.release();
    d_vDispBinary.release();
    FreeBatch();
    m_is_initialized = false;
}

void RoadEstimation::FreeBatch() { /* (under the caller's device guard) */
    IS_CHECK_RETURN(is_road_ctx_destroy(m_batch_ctx)); /* synchronises the device */
    d_batch_out.release();
    h_batch_out.release();
    m_batch_ctx = nullptr;
    m_batch_cap = m_batch_out_lines = 0;
}

void RoadEstimation::SetBatchLimits(int max_lines, int max_candidates) {
    if (max_lines < 1) throw std::invalid_argument("max_lines must be at least 1");
    if (max_candidates < 1 || max_candidates > IS_ROAD_MAX_CANDIDATES)
        throw std::invalid_argument("max_candidates outside [1, IS_ROAD_MAX_CANDIDATES]");
    m_batch_lines = max_lines;
    m_batch_candidates = max_candidates;
}

/* out block, in the order that lets ONE copy fetch n frames: [cap] totals, [cap] overflow flags, [cap][L][2] lines */
void RoadEstimation::ReserveBatch(int n_images) { /* (under the caller's device guard) */
    const int L = m_batch_lines;
    if (n_images > m_batch_cap || L != m_batch_out_lines) {
        const int cap = std::max(n_images, m_batch_cap);
        FreeBatch();
        IS_CHECK_RETURN(is_road_ctx_create(&m_batch_ctx, m_rows, m_cols, m_max_dis, cap, m_ctx_device));
        const size_t bytes = sizeof(int) * 2 * (size_t)cap + sizeof(float) * 2 * (size_t)cap * L;
        d_batch_out.reserve(bytes);
        h_batch_out.reserve(bytes);
        m_batch_cap = cap;
        m_batch_out_lines = L;
    }
}

/* What ComputeBatch and ComputeBatchDevice share (under the caller's device guard): their refusals, the stream choice,
 * the scratch, and v-disparity + Hough transform of the batch queued on that stream. */
RoadEstimation::BatchLines RoadEstimation::EnqueueBatch(const char* who, const pixel_t* d_im, int n_images,
                                                        bool outputs, void* stream) {
    if (!m_is_initialized) throw std::invalid_argument(std::string("RoadEstimation::") + who + " before Initialize()");
    if (n_images < 1 || !d_im || !outputs) throw std::invalid_argument(std::string(who) + ": empty batch or null pointer");
    ReserveBatch(n_images);
    BatchLines q;
    q.stream = stream ? stream : m_stream;
    q.d_total = (int*)d_batch_out.get();
    q.d_overflow = q.d_total + m_batch_cap;
    q.d_lines = (float*)(q.d_overflow + m_batch_cap);
    IS_CHECK_RETURN(is_road_vdisparity_batch(m_batch_ctx, d_im, n_images, m_binThr, nullptr, nullptr, nullptr, q.stream));
    IS_CHECK_RETURN(is_road_hough_batch(m_batch_ctx, n_images, m_HoughAccumThr, m_batch_lines, m_batch_candidates,
                                        q.d_lines, nullptr, q.d_total, q.d_overflow, q.stream));
    return q;
}

void RoadEstimation::ComputeBatchDevice(const pixel_t* d_im, int n_images, Stixels::RoadParameters* d_road,
                                        uint8_t* d_status, const Stixels::RoadParameters& fallback, void* stream) {
    const DeviceGuard guard(m_ctx_device);
    const BatchLines q = EnqueueBatch("ComputeBatchDevice", d_im, n_images, d_road && d_status, stream);
    static_assert(sizeof(Stixels::RoadParameters) == sizeof(is_road_params), "d_road holds is_road_params records");
    const is_road_params fb = {fallback.vhor, fallback.camera_tilt, fallback.camera_height, fallback.alpha_ground};
    IS_CHECK_RETURN(is_road_choose_batch(m_batch_ctx, n_images, q.d_lines, q.d_total, q.d_overflow, m_batch_lines, m_cy,
                                         m_b, m_focal, m_minPitch, m_maxPitch, fb, (is_road_params*)d_road, d_status,
                                         q.stream));
}

void RoadEstimation::PitchGate(float& min_pitch, float& max_pitch) {
    max_pitch = 50 * kPi / 180.0f; /* RE.cu:47-57 */
    min_pitch = -50 * kPi / 180.0f;
}

int RoadEstimation::ChooseLineShared(float camera_center_y, float baseline, float focal, int rows, float min_pitch,
                                     float max_pitch, const float* lines, int total, int overflow, int max_lines,
                                     const Stixels::RoadParameters& fallback, Stixels::RoadParameters& out,
                                     int* index) { /* k_road_choose, line by line */
    const float step = IS_ROAD_HOUGH_THETA;
    const int numangle = is_hough_numangle(step);
    out = fallback;
    if (index) *index = -1;
    const int nl = overflow ? 0 : std::min(total, max_lines);
    for (int k = 0; k < nl; k++) {
        const float rho = std::abs(lines[2 * k]);
        const float theta = lines[2 * k + 1];
        const int n = is_road_angle_index(theta, step, numangle);
        if (n < 0) continue;
        const float line_theta = 0.0f + n * step; /* (== theta; the expression of the device's table) */
        is_road_params r = {0, 0.0f, 0.0f, 0.0f};
        int vhor_ok = 0;
        if (!is_road_line(rho, sinf(line_theta), cosf(line_theta), camera_center_y, baseline, focal, rows, min_pitch,
                          max_pitch, &r, &vhor_ok))
            continue;
        if (index) *index = k;
        if (!vhor_ok) return IS_ROAD_HORIZON;
        out = Stixels::RoadParameters{r.vhor, r.tilt, r.height, r.alpha};
        return IS_ROAD_OK;
    }
    return overflow || total > max_lines ? IS_ROAD_UNDECIDED : IS_ROAD_NONE;
}

void RoadEstimation::ComputeBatch(const pixel_t* d_im, int n_images, Stixels::RoadParameters* out, uint8_t* ok,
                                  void* stream) {
    const DeviceGuard guard(m_ctx_device);
    void* s = EnqueueBatch("ComputeBatch", d_im, n_images, out && ok, stream).stream;
    const int L = m_batch_lines, cap = m_batch_cap;
    const size_t bytes = sizeof(int) * 2 * (size_t)cap + sizeof(float) * 2 * (size_t)n_images * L;
    IS_CHECK_RETURN(is_memcpy_d2h(h_batch_out.get(), d_batch_out.get(), bytes, s));
    IS_CHECK_RETURN(is_stream_synchronize(s));

    const int* total = (const int*)h_batch_out.get();
    const int* overflow = total + cap;
    const float* h_lines = (const float*)(overflow + cap);
    const size_t cells = (size_t)m_rows * m_max_dis;
    std::vector<std::pair<float, float>> lines;
    m_batch_fallbacks = 0;
    for (int i = 0; i < n_images; i++) {
        const int nl = std::min(total[i], L);
        lines.resize(nl);
        for (int k = 0; k < nl; k++)
            lines[k] = std::make_pair(h_lines[((size_t)i * L + k) * 2], h_lines[((size_t)i * L + k) * 2 + 1]);
        bool found = !overflow[i] && ChooseLine(lines.data(), lines.size(), out[i]) >= 0;
        if (!found && (overflow[i] || total[i] > L)) { /* the lines the device kept do not decide it */
            lines = FetchHoughLines(is_road_ctx_binary(m_batch_ctx) + i * cells, m_batch_binary, s);
            found = ChooseLine(lines.data(), lines.size(), out[i]) >= 0;
            m_batch_fallbacks++;
        }
        ok[i] = found ? 1 : 0;
        if (!found) out[i] = Stixels::RoadParameters{0, 0.0f, 0.0f, 0.0f};
    }
}

int RoadEstimation::ChooseLine(float camera_center_y, float baseline, float focal, int rows,
                               const std::pair<float, float>* lines, size_t n, Stixels::RoadParameters& out) {
    RoadEstimation re; /* (no device buffers: never initialised) */
    re.SetCamera(camera_center_y, baseline, focal, rows);
    return re.ChooseLine(lines, n, out);
}

int RoadEstimation::ChooseLine(const std::pair<float, float>* lines, size_t n,
                               Stixels::RoadParameters& out) const { /* RE.cu:155-176 */
    float rho, theta, horizonPoint, pitch, cameraHeight, slope;
    for (size_t k = 0; k < n; k++) {
        rho = std::abs(lines[k].first);
        theta = lines[k].second;
        ComputeCameraProperties(m_rows, rho, theta, horizonPoint, pitch, cameraHeight, slope);
        if (pitch >= m_minPitch && pitch <= m_maxPitch) {
            out = Stixels::RoadParameters{(int)ceil(horizonPoint), pitch, cameraHeight, slope};
            return (int)k;
        }
    }
    return -1;
}

bool RoadEstimation::Compute(const std::vector<pixel_t>& im) { /* RE.cu:94-102 */
    {
        const DeviceGuard guard(m_ctx_device);
        IS_CHECK_RETURN(is_memcpy_h2d(d_disparity.get(), im.data(), im.size() * sizeof(pixel_t), m_stream));
        IS_CHECK_RETURN(is_stream_synchronize(m_stream)); /* the caller's vector may be a temporary */
    }
    return Compute(d_disparity.get());
}

bool RoadEstimation::Compute(pixel_t* d_im) { /* RE.cu:104-138 */
    const DeviceGuard guard(m_ctx_device); /* (d_im lives on the object's device: Stixels::SetDevice(d) + SetDevice(d)) */
    IS_CHECK_RETURN(is_road_vdisparity(d_im, m_rows, m_cols, m_max_dis, m_binThr, d_vDisp.get(), d_maximum.get(),
                                       d_vDispBinary.get(), m_stream));
    const auto lines = FetchHoughLines(d_vDispBinary.get(), m_vDisp, m_stream); /* RE.cu:140-153 */
    Stixels::RoadParameters r;
    const int k = ChooseLine(lines.data(), lines.size(), r);
    if (k < 0) return false;
    m_rho = std::abs(lines[k].first);
    m_theta = lines[k].second;
    m_horizonPoint = r.vhor;
    m_pitch = r.camera_tilt;
    m_cameraHeight = r.camera_height;
    m_slope = r.alpha_ground;
    return true;
}

std::vector<std::pair<float, float>> RoadEstimation::FetchHoughLines(const uint8_t* d_binary,
                                                                     std::vector<uint8_t>& image, void* stream) {
    image.resize((size_t)m_max_dis * m_rows);
    IS_CHECK_RETURN(is_memcpy_d2h(image.data(), d_binary, image.size(), stream));
    IS_CHECK_RETURN(is_stream_synchronize(stream));
    return HoughLines(image.data(), m_rows, m_max_dis, IS_ROAD_HOUGH_RHO, IS_ROAD_HOUGH_THETA, m_HoughAccumThr);
}

/* OpenCV's HoughLinesStandard (the algorithm behind cv::HoughLines(image, lines, rho, theta,
 * threshold)): accumulator of (numangle+2) x (numrho+2) cells, votes for every non-zero pixel,
 * 4-neighbour local maxima above the threshold, sorted by votes. */
std::vector<std::pair<float, float>> RoadEstimation::HoughLines(const uint8_t* image, int rows,
                                                                int cols, float rho, float theta,
                                                                int threshold) {
    const int width = cols, height = rows;
    const float min_theta = 0;
    const int numangle = is_hough_numangle(theta), numrho = is_hough_numrho(width, height, rho);
    std::vector<int> accum((size_t)(numangle + 2) * (numrho + 2), 0);
    std::vector<float> tabSin(numangle), tabCos(numangle);
    is_hough_tables(numangle, rho, theta, tabSin.data(), tabCos.data());
    for (int i = 0; i < height; i++)
        for (int j = 0; j < width; j++)
            if (image[(size_t)i * width + j] != 0)
                for (int n = 0; n < numangle; n++) {
                    int r = (int)lrint(j * tabCos[n] + i * tabSin[n]);
                    r += (numrho - 1) / 2;
                    accum[(size_t)(n + 1) * (numrho + 2) + r + 1]++;
                }
    std::vector<int> sort_buf;
    for (int r = 0; r < numrho; r++)
        for (int n = 0; n < numangle; n++) {
            const int base = (n + 1) * (numrho + 2) + r + 1;
            if (accum[base] > threshold && accum[base] > accum[base - 1] &&
                accum[base] >= accum[base + 1] && accum[base] > accum[base - numrho - 2] &&
                accum[base] >= accum[base + numrho + 2])
                sort_buf.push_back(base);
        }
    std::sort(sort_buf.begin(), sort_buf.end(), [&](int l1, int l2) {
        return accum[l1] > accum[l2] || (accum[l1] == accum[l2] && l1 < l2);
    });
    std::vector<std::pair<float, float>> lines;
    const double scale = 1. / (numrho + 2);
    for (int idx : sort_buf) {
        const int n = (int)floor(idx * scale) - 1;
        const int r = idx - (n + 1) * (numrho + 2) - 1;
        lines.emplace_back((r - (numrho - 1) * 0.5f) * rho, min_theta + n * theta);
    }
    return lines;
}

void RoadEstimation::ComputeCameraProperties(int vdisp_rows, const float rho, const float theta,
                                             float& horizonPoint, float& pitch,
                                             float& cameraHeight, float& slope) const { /* :178-193 */
    horizonPoint = rho / sinf(theta);
    pitch = -atanf((m_cy - horizonPoint) / (m_focal)); /* y axis is inverted */
    const float last_row = (float)(vdisp_rows - 1);
    const float vDispDown = (rho - last_row * sinf(theta)) / cosf(theta);
    slope = (0 - vDispDown) / (horizonPoint - last_row);
    cameraHeight = m_b * cosf(pitch) / slope;
}
