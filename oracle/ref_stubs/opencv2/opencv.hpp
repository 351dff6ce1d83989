/*
 * Stand-in for OpenCV's umbrella header, for the one translation unit of the reference that includes it
 * (RoadEstimation.cu).  TEST INFRASTRUCTURE ONLY, of this project's own writing.
 *
 * It declares only what that translation unit names: cv::Mat (rows, cols, data pointer and the constructor over
 * caller-owned memory), cv::Vec2f, CV_PI, CV_8UC1 and cv::HoughLines.  This HoughLines holds NO transform: it
 * records what it was called with -- a copy of the image, its shape and type, rho, theta, threshold -- and returns
 * the line list that the driver installed beforehand (oracle/ref_driver.hip: ref_road_set_lines).  The tests feed it
 * the lines of this project's own transform, or hand-made lists, and so compare everything AROUND the transform
 * -- the v-disparity kernels, the call's arguments, the line choice, the camera properties -- with the reference's
 * own code.
 */
#ifndef REF_STUBS_OPENCV2_OPENCV_HPP_
#define REF_STUBS_OPENCV2_OPENCV_HPP_

#include <cstddef>
#include <vector>

#define CV_PI 3.1415926535897932384626433832795
#define CV_8UC1 0

namespace cv {

struct Mat {
    int rows, cols, type;
    unsigned char* data;
    Mat(int rows_, int cols_, int type_, void* data_)
        : rows(rows_), cols(cols_), type(type_), data(static_cast<unsigned char*>(data_)) {}
};

struct Vec2f {
    float val[2];
    float& operator[](int i) { return val[i]; }
    const float& operator[](int i) const { return val[i]; }
};

/* What the last HoughLines call saw, and what the next one returns. */
struct HoughLinesStub {
    std::vector<Vec2f> answer;
    std::vector<unsigned char> image;
    int rows = 0, cols = 0, type = -1, threshold = 0, calls = 0;
    double rho = 0, theta = 0;
};

inline HoughLinesStub& hough_lines_stub() {
    static HoughLinesStub stub;
    return stub;
}

inline void HoughLines(const Mat& image, std::vector<Vec2f>& lines, double rho, double theta, int threshold) {
    HoughLinesStub& s = hough_lines_stub();
    const std::size_t n = (image.rows > 0 && image.cols > 0 && image.data) ? (std::size_t)image.rows * image.cols : 0;
    s.image.assign(image.data, image.data + n);
    s.rows = image.rows; s.cols = image.cols; s.type = image.type;
    s.rho = rho; s.theta = theta; s.threshold = threshold;
    s.calls++;
    lines = s.answer;
}

}  // namespace cv

#endif
