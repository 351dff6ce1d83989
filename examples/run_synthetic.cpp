/*
 * run_synthetic.cpp -- a plain C++ caller of the drop-in `Stixels` / `RoadEstimation` classes,
 * following the call sequence of the reference's apps/run_cityscapes.cu:245-449 (SetConfig ->
 * Initialize -> per frame: SetDisparityImage, SetSegmentation, RoadEstimation::Compute,
 * SetRoadParameters, Compute, GetInstanceStixels, SaveStixels -> Finish) on a synthetic frame
 * (there is no dataset, PNG/HDF5 reader or CNN in this image).  Note: no device code and no HIP
 * header in this translation unit -- it is compiled by g++ and linked against
 * libInstanceStixels.so.
 *
 *   g++ -std=c++17 -O2 -Iinclude -Iinclude/InstanceStixels examples/run_synthetic.cpp \
 *       -Linstance_stixels_amd/lib -lInstanceStixels -lis_core \
 *       -Wl,-rpath,$PWD/instance_stixels_amd/lib -o examples/run_synthetic
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "RoadEstimation.h"
#include "Stixels.hpp"

int main(int argc, char** argv) {
    const int rows = argc > 1 ? atoi(argv[1]) : 1024;
    const int cols = argc > 2 ? atoi(argv[2]) : 2048;
    const int max_dis = argc > 3 ? atoi(argv[3]) : 128;
    const bool pairwise = argc > 4 ? atoi(argv[4]) != 0 : false;
    const int frames = argc > 5 ? atoi(argv[5]) : 10;

    StixelConfig cfg; /* run_cityscapes.cu:184-198 + camera.json values */
    cfg.rows = rows; cfg.cols = cols; cfg.max_dis = max_dis;
    cfg.column_step = 8;
    cfg.invalid_disparity = -1.0f;
    cfg.n_semantic_classes = 19; cfg.n_offset_channels = 2;
    cfg.prior_weight = pairwise ? 1.0f : 1e4f;
    cfg.segmentation_weight = pairwise ? 4.7095f : 11.241965f;
    cfg.instance_weight = pairwise ? 0.003131f : 0.001731f;
    cfg.disparity_weight = pairwise ? 0.0001f : 0.006993f;
    cfg.eps = 23.89408f; cfg.min_pts = 4; cfg.size_filter = 42;
    cfg.focal = 2262.52f; cfg.baseline = 0.209313f;
    cfg.camera_center_x = 0.5f * cols; cfg.camera_center_y = 0.5f * rows;

    /* synthetic frame: ground ramp below the horizon, one object slab, sky */
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const int vhor_img = (int)(0.45f * rows);
    const float alpha = 0.8f * max_dis / (rows - vhor_img);
    std::vector<pixel_t> disp((size_t)rows * cols);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            float d = r > vhor_img ? alpha * (r - vhor_img) + U(rng) : 0.5f * U(rng);
            if (c > cols / 3 && c < cols / 2 && r > rows / 3 && r < 3 * rows / 4)
                d = alpha * (3 * rows / 4 - vhor_img) + U(rng);
            disp[(size_t)r * cols + c] = std::fmin(std::fmax(d, 0.01f), max_dis - 1.01f);
        }
    const int realcols = cols / 8;
    const int p2s = (int)powf(2, ceilf(log2f(rows / 8 + 1)));
    std::vector<int32_t> seg((size_t)realcols * 21 * p2s, 0);
    for (int c = 0; c < realcols; c++)
        for (int ch = 0; ch < 19; ch++)
            for (int k = 0; k < rows / 8; k++) { /* k = 0 is the image bottom */
                const int img_row = rows - 1 - (8 * k + 4);
                const bool obj = 8 * c > cols / 3 && 8 * c < cols / 2 && img_row > rows / 3 &&
                                 img_row < 3 * rows / 4;
                const int truth = obj ? 13 : (img_row > vhor_img ? 0 : 10);
                seg[((size_t)c * 21 + ch) * p2s + k] = (ch == truth ? 1 : 30) + (int)(4 * U(rng));
            }

    Stixels stixels;
    RoadEstimation road;
    stixels.SetConfig(cfg);
    stixels.Initialize();
    road.Initialize(cfg.camera_center_y, cfg.baseline, cfg.focal, rows, cols, max_dis);
    StixelsData data;
    double total_ms = 0;
    for (int f = 0; f < frames; f++) {
        stixels.SetDisparityImage(disp);
        const auto t0 = std::chrono::steady_clock::now();
        stixels.SetSegmentation(seg);
        if (!road.Compute(stixels.GetInputDisparityImageOnDevice())) {
            printf("Road estimation failed.\n");
            return 1;
        }
        stixels.SetRoadParameters(road.GetHorizonPoint(), road.GetPitch(), road.GetCameraHeight(),
                                  road.GetSlope());
        stixels.Compute(pairwise, data);
        const auto t1 = std::chrono::steady_clock::now();
        if (f > 0) total_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    auto mapping = stixels.GetInstanceStixels();
    int n_stixels = 0;
    for (int c = 0; c < data.realcols; c++)
        for (int i = 0; i < data.max_sections && data.sections[(size_t)c * data.max_sections + i].type != -1; i++)
            n_stixels++;
    Stixels::SaveStixels(data.sections.data(), mapping, road.GetSlope(), data.vhor,
                         stixels.GetRealCols(), stixels.GetMaxSections(), "/tmp/synthetic.stixels");
    printf("horizon row %d (generated %d), slope %.4f (generated %.4f)\n", road.GetHorizonPoint(),
           vhor_img, road.GetSlope(), alpha);
    printf("%d stixels, %zu instance candidates; it took an average of %.3f milliseconds, %.1f fps\n",
           n_stixels, mapping.size(), total_ms / (frames - 1), 1000.0 * (frames - 1) / total_ms);
    /* the same frame per instance instead of per stixel, reduced on the device */
    const Stixels::InstanceObjectsView objects = stixels.InstanceObjectsBatchView(1);
    printf("%d instance objects with %d contour points\n", objects.n_objects, objects.n_points);
    stixels.Finish();
    road.Finish();
    return 0;
}
