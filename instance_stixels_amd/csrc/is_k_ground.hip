/*
 * is_k_ground.hip -- the ground model of a batch on the device: Stixels::PrecomputeGround for n frames, from road
 * records that never left the device (is_road_choose_batch), into the arrays the DP kernels read.  The arithmetic
 * is is_ground_row (is_ground_model.h), the source Stixels::PrecomputeGroundShared compiles on the host: bitwise
 * equal by construction.  See is_compute_road in instance_stixels_core.h.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "is_ground_model.h"
#include "is_launch.h"

/* One thread per (row, frame): ground [n][3][rows] = function | normalization | inv_sigma2, vhor [n] = the library-
 * convention horizon rows - vhor_image - 1.  The log table is gathered with a clamped index (is_fast_log_index). */
__global__ __launch_bounds__(256) void k_ground_model(is_ground_params g, const float* __restrict__ log_lut,
                                                      int lut_entries, const is_road_params* __restrict__ road,
                                                      float* __restrict__ ground, int* __restrict__ vhor, int rows) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= rows) return;
    const is_road_params r = road[f];
    const int vhor_lib = rows - r.vhor - 1;
    float fn, norm, is2;
    is_ground_row(&g, log_lut, lut_entries, vhor_lib, r.tilt, r.height, r.alpha, v, &fn, &norm, &is2, nullptr);
    float* dst = ground + (size_t)f * 3 * rows;
    dst[v] = fn;
    dst[rows + v] = norm;
    dst[2 * rows + v] = is2;
    if (v == 0) vhor[f] = vhor_lib;
}

extern "C" hipError_t isk_launch_ground_model(const is_ground_params* g, const float* log_lut, int lut_entries,
                                              const is_road_params* road, float* ground, int* vhor, int n_images,
                                              int rows, hipStream_t stream) {
    hipLaunchKernelGGL(k_ground_model, dim3((rows + 255) / 256, n_images), dim3(256), 0, stream, *g, log_lut,
                       lut_entries, road, ground, vhor, rows);
    return hipGetLastError();
}
