/*
 * ground_device_main.cpp -- stand-alone driver (its own main) of the host code of the device-resident road chain,
 * for a build with -fsanitize=undefined,address (tests/test_ground_device_cpu.py builds and runs it): no GPU, no
 * device call.  RoadEstimation::ChooseLineShared over hostile line lists -- theta = 0 (rho / 0), rho = 0, NaN and
 * infinities, thetas that are no table angle, horizons far outside the image -- and is_ground_row over hostile roads.
 * Any float -> int conversion out of range, any index outside the log table, stops the program.
 */
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "InstanceStixels/RoadEstimation.h"
#include "is_ground_model.h"

static int fail(const char* what) {
    std::printf("ground_device_main: FAILED: %s\n", what);
    return 1;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float step = 3.1415926535897932384626433832795f / 180;
    const float rhos[] = {0.0f, -0.0f, 1e-45f, 1.0f, 100.0f, -100.0f, 5000.0f, 3e38f, -3e38f, inf, -inf, nan};
    std::vector<float> thetas;
    for (int n = -1; n <= 181; n++) thetas.push_back(0.0f + n * step);
    for (float t : {nan, inf, -inf, 1.0f, 1e-45f, 3e38f, -3e38f, std::nextafter(90 * step, 0.0f)}) thetas.push_back(t);
    std::vector<float> lines;
    for (float r : rhos)
        for (float t : thetas) { lines.push_back(r); lines.push_back(t); }
    const int total = (int)(lines.size() / 2);
    float lo, hi;
    RoadEstimation::PitchGate(lo, hi);
    const Stixels::RoadParameters fb = {11, 0.125f, 1.5f, 0.25f};
    int seen[4] = {0, 0, 0, 0};
    const float cameras[][3] = {{128.0f, 0.2f, 700.0f}, {0.0f, 0.0f, 0.0f}, {-1e30f, 1e30f, 1e-30f}, {nan, nan, nan}};
    for (const auto& cam : cameras)
        for (int rows : {1, 2, 256, 32767})
            for (int first = 0; first < total; first++) { /* every line heads a list once */
                Stixels::RoadParameters out;
                int index = -2;
                const int st = RoadEstimation::ChooseLineShared(cam[0], cam[1], cam[2], rows, lo, hi,
                                                                lines.data() + 2 * first, total - first, 0, 3, fb, out,
                                                                &index);
                if (st < 0 || st > 3) return fail("status outside [0, 3]");
                seen[st]++;
                if (st == IS_ROAD_OK) {
                    if (index < 0 || out.vhor < 0 || out.vhor >= rows) return fail("an accepted horizon outside the image");
                } else if (out.vhor != fb.vhor || out.camera_tilt != fb.camera_tilt ||
                           out.camera_height != fb.camera_height || out.alpha_ground != fb.alpha_ground) {
                    return fail("no fallback where the status is not IS_ROAD_OK");
                }
            }
    if (!seen[0] || !seen[1] || !seen[2] || !seen[3]) return fail("a status value never occurred");
    {   /* an overflowed frame looks at no line; negative totals are empty lists */
        Stixels::RoadParameters out;
        if (RoadEstimation::ChooseLineShared(128.0f, 0.2f, 700.0f, 256, lo, hi, nullptr, 5, 1, 4, fb, out) !=
            IS_ROAD_UNDECIDED)
            return fail("overflow");
        if (RoadEstimation::ChooseLineShared(128.0f, 0.2f, 700.0f, 256, lo, hi, nullptr, -7, 0, 4, fb, out) != IS_ROAD_NONE)
            return fail("negative total");
    }

    /* the ground rows: a table of exactly lut_entries floats on the heap, so that ASan sees any index beside it */
    const int entries = 1000 + 1;
    std::vector<float> lut(entries);
    for (int i = 0; i < entries; i++) lut[i] = std::log((float)i / (entries - 1));
    const is_ground_params g = {700.0f, 0.2f, 64.0f, 0.15f, 1.0f, 0.05f, 0.05f * 3.1416f / 180.0f};
    const float vals[] = {0.0f, -0.0f, 1e-45f, 1e-30f, 0.01f, 1.5f, -1.5f, 3e38f, -3e38f, inf, -inf, nan};
    const int vhors[] = {0, 100, -1, 255, 1 << 30, -(1 << 30), std::numeric_limits<int>::min() + 300,
                         std::numeric_limits<int>::max()};
    long rows_done = 0;
    for (int vh : vhors)
        for (float tilt : vals)
            for (float height : vals)
                for (float alpha : vals)
                    for (int v : {0, 1, 128, 255}) {
                        float fn, norm, is2;
                        int idx = -1;
                        is_ground_row(&g, lut.data(), entries, vh, tilt, height, alpha, v, &fn, &norm, &is2, &idx);
                        if (idx < 0 || idx >= entries) return fail("FastLog index outside the table");
                        rows_done++;
                    }
    std::printf("ground_device_main: ok (%d line lists per camera and image height, status counts %d %d %d %d; %ld ground rows)\n",
                total, seen[0], seen[1], seen[2], seen[3], rows_done);
    return 0;
}
