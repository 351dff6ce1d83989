/*
 * RoadEstimation.h -- road / camera-pose estimation from the v-disparity histogram, source-
 * compatible with /root/reference/InstanceStixels/include/InstanceStixels/RoadEstimation.h:32-94
 * (same public methods) but without OpenCV: the reference calls cv::HoughLines on the
 * binarised histogram (RoadEstimation.cu:153); here the standard Hough transform is implemented
 * in RoadEstimation.cpp following OpenCV's published HoughLinesStandard algorithm
 * (rho = 1, theta = pi/180, accumulator threshold 25, lines sorted by votes).
 */
#ifndef INSTANCESTIXELS_AMD_ROADESTIMATION_H_
#define INSTANCESTIXELS_AMD_ROADESTIMATION_H_

#include <stdint.h>

#include <vector>

#include "Stixels.hpp"
#include "configuration.h"
#include "util.h"

class RoadEstimation {
public:
    RoadEstimation();
    ~RoadEstimation();

    void Initialize(const float camera_center_y, const float baseline, const float focal,
                    const int rows, const int cols, const int max_dis,
                    const float road_vdisparity_threshold = 0.2f);
    void Finish();

    bool Compute(const std::vector<pixel_t>& im);
    bool Compute(pixel_t* d_im);

    float GetCameraHeight() { return m_cameraHeight; }
    float GetPitch() { return m_pitch; }
    float GetSlope() { return m_slope; }
    int GetHorizonPoint() { return m_horizonPoint; }
    bool IsInitialized() { return m_is_initialized; }

    /* ---- additions (not in the reference) ----
     * Device the next Initialize() allocates on; default (-1): the calling thread's current HIP
     * device at Initialize() time.  Every later call (Compute, Finish) runs on that device
     * whatever the caller's current device is, on a stream of the object's own (an ordinary stream
     * that synchronises with the legacy NULL stream, like Stixels): together with
     * Stixels::SetDevice(d) the wrapper sequence GetInputDisparityImageOnDevice() ->
     * RoadEstimation::Compute(ptr) (apps/stixels_wrapper.cu:187) stays on device d. */
    void SetDevice(int device) { m_device = device; }
    int GetDevice() const { return m_device; }
    int GetActiveDevice() const { return m_ctx_device; }

    /* Batched road estimation (an addition): the result of Compute(d_disparity + i * rows * cols) for every frame
     * i of d_disparity [n_images][rows][cols] (device, on the object's device), bit for bit, written as the
     * road parameters of Stixels::ComputeBatch:
     *   out[i] = {(int)ceil(horizon point), pitch, camera height, slope} and ok[i] = 1 where Compute would
     *   return true; out[i] = {0, 0, 0, 0} and ok[i] = 0 where it would return false.
     * The histogram and the Hough transform of the whole batch run on the device (is_road_vdisparity_batch,
     * is_road_hough_batch), the lines come back in one copy, and the line choice of Compute runs on the host.
     * A frame whose candidate buffer overflowed, or whose first max_lines lines hold no acceptable one while it
     * has more, is finished with HoughLines on its binary image (GetBatchFallbacks()).  `stream`: a hipStream_t
     * of the object's device, or null for the object's own stream; the call returns after it synchronised
     * once.  Device scratch for n_images frames is allocated on first need and released by Finish().  The
     * single-frame getters (GetPitch() ...) are left as they are. */
    void ComputeBatch(const pixel_t* d_disparity, int n_images, Stixels::RoadParameters* out, uint8_t* ok,
                      void* stream = nullptr);
    /* The same estimation with the line choice on the device and NOTHING returned to the host (an addition):
     * v-disparity, Hough transform and is_road_choose_batch are queued on `stream`; no copy, no synchronisation.
     *   d_road   [n_images] Stixels::RoadParameters, d_status [n_images] uint8 (IS_ROAD_* of
     *            instance_stixels_core.h), both on the object's device: what Stixels::ComputeBatchRoad consumes
     *   fallback the record of every frame whose status is not IS_ROAD_OK (no line, undecided, horizon outside
     *            the image): the DP of such a frame then runs on defined numbers, and the status tells the caller
     * The choice is ChooseLineShared's, bit for bit.  Against ComputeBatch: the same line, vhor and alpha; tilt
     * within 1 ulp and height within 2 ulp (is_atanf / is_cosf in place of libm's).  An undecided frame
     * (IS_ROAD_UNDECIDED: ComputeBatch would re-run HoughLines on its binary image) is reported, not finished. */
    void ComputeBatchDevice(const pixel_t* d_disparity, int n_images, Stixels::RoadParameters* d_road,
                            uint8_t* d_status, const Stixels::RoadParameters& fallback, void* stream = nullptr);
    /* Lines returned per frame (default 256) and local maxima kept per frame (default 4096, at most
     * IS_ROAD_MAX_CANDIDATES) by the device Hough transform of ComputeBatch. */
    void SetBatchLimits(int max_lines, int max_candidates);
    /* Frames of the last ComputeBatch that were finished with the host Hough transform. */
    int GetBatchFallbacks() const { return m_batch_fallbacks; }

    /* additions for tests */
    const std::vector<uint8_t>& GetBinaryVDisparity() const { return m_vDisp; }
    /* Standard Hough transform of a rows x cols 8-bit image; returns (rho, theta) pairs sorted
     * by accumulator votes (descending, ties by accumulator index). */
    static std::vector<std::pair<float, float>> HoughLines(const uint8_t* image, int rows, int cols,
                                                           float rho, float theta, int threshold);
    /* The line choice of Compute / ComputeBatch on a given list, for a camera and a v-disparity image of `rows`
     * rows, without a device: the index of the first line whose pitch passes the gate (out = its road
     * parameters), or -1 (out untouched). */
    static int ChooseLine(float camera_center_y, float baseline, float focal, int rows,
                          const std::pair<float, float>* lines, size_t n, Stixels::RoadParameters& out);

    /* The host twin of is_road_choose_batch, without a device: ChooseLine with is_atanf / is_cosf of is_numerics.h
     * in place of atanf / cosf(pitch), over the first min(total, max_lines) lines of `lines` [.][2] (rho, theta) as
     * is_road_hough_batch leaves them, with the gate [min_pitch, max_pitch].  Returns the status (IS_ROAD_*) and
     * sets out = the accepted line's record (IS_ROAD_OK) or `fallback`; *index (may be null) = the accepted
     * line's index or -1.  A line whose theta is not 0.0f + n * (float)pi / 180 for 0 <= n < 180 is skipped. */
    static int ChooseLineShared(float camera_center_y, float baseline, float focal, int rows, float min_pitch,
                                float max_pitch, const float* lines, int total, int overflow, int max_lines,
                                const Stixels::RoadParameters& fallback, Stixels::RoadParameters& out,
                                int* index = nullptr);
    /* the pitch gate of Initialize() (what ComputeBatchDevice passes) */
    static void PitchGate(float& min_pitch, float& max_pitch);

private:
    /* the output blocks of the batched transforms for n_images frames (allocated on first need, grown on demand) */
    void ReserveBatch(int n_images);
    /* the camera and the pitch gate of Initialize (everything the line choice reads) */
    void SetCamera(float camera_center_y, float baseline, float focal, int rows);
    void ComputeCameraProperties(int vdisp_rows, const float rho, const float theta,
                                 float& horizonPoint, float& pitch, float& cameraHeight,
                                 float& slope) const;
    /* the line choice of Compute over lines[0 .. n): the index of the accepted line (out = its record), or -1 */
    int ChooseLine(const std::pair<float, float>* lines, size_t n, Stixels::RoadParameters& out) const;
    /* HoughLines of a binary v-disparity image on the device, fetched into `image` (one synchronisation) */
    std::vector<std::pair<float, float>> FetchHoughLines(const uint8_t* d_binary, std::vector<uint8_t>& image,
                                                         void* stream);
    /* v-disparity + Hough transform of a batch, queued: where in d_batch_out its lines land, and the stream */
    struct BatchLines { int* d_total; int* d_overflow; float* d_lines; void* stream; };
    BatchLines EnqueueBatch(const char* who, const pixel_t* d_disparity, int n_images, bool outputs, void* stream);
    void FreeBatch();

    bool m_is_initialized = false;
    int m_device = -1;      /* requested (SetDevice) */
    int m_ctx_device = -1;  /* where the buffers of the last Initialize() live */
    void* m_stream = nullptr;
    DeviceArray<pixel_t> d_disparity;
    DeviceArray<int> d_vDisp;
    DeviceArray<int> d_maximum;
    DeviceArray<uint8_t> d_vDispBinary;
    std::vector<uint8_t> m_vDisp;
    /* ComputeBatch */
    is_road_ctx* m_batch_ctx = nullptr; /* scratch for m_batch_cap frames */
    int m_batch_cap = 0;
    int m_batch_lines = 256, m_batch_candidates = 4096;
    int m_batch_out_lines = 0;          /* max_lines the output blocks below were sized for */
    DeviceArray<char> d_batch_out;      /* [cap] totals, [cap] overflow flags, [cap][lines][2] float lines */
    PinnedArray<char> h_batch_out;      /* pinned twin of d_batch_out */
    int m_batch_fallbacks = 0;
    std::vector<uint8_t> m_batch_binary;

    int m_HoughAccumThr = 25;
    float m_binThr = 0.2f, m_maxPitch = 0, m_minPitch = 0;
    float m_maxCameraHeight = 0, m_minCameraHeight = 0;
    int m_max_dis = 0, m_rows = 0, m_cols = 0;
    float m_rho = 0, m_theta = 0;
    int m_horizonPoint = 0;
    float m_pitch = 0, m_cameraHeight = 0, m_cy = 0, m_b = 0, m_focal = 0, m_slope = 0;
};

#endif
