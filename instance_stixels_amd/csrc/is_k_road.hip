/*
 * is_k_road.hip -- road estimation (f3), for one frame and for n: v-disparity histogram, binarisation (+
 * compaction), the standard Hough transform and its per-frame sort, every launch covering the whole batch.
 * Results are those of RoadEstimation::Compute frame by frame (the same histogram kernels, and
 * RoadEstimation::HoughLines for the transform), bit for bit.  See is_road_* in instance_stixels_core.h.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "is_ground_model.h"
#include "is_launch.h"

/* Per-frame counters of the batch scratch: [frame][IS_ROAD_CNT] ints. */
#define IS_ROAD_CNT 2
#define IS_ROAD_CNT_MAX 0    /* maximum of the histogram */
#define IS_ROAD_CNT_POINTS 1 /* non-zero pixels of the binary image (entries of the point list) */
#define IS_ROAD_SORT_MAX 8192 /* largest candidate capacity the one-workgroup sort handles (64 KiB of keys) */

/* f3: v-disparity histogram, maximum, binarisation (RoadEstimationKernels.cu:25-60), of the single-frame entry
 * (is_road_vdisparity: a batch of one whose counters are the caller's maximum) and of the batched one.
 * The reference does one global atomicAdd per pixel and a second kernel of global atomicMax.  Here one workgroup
 * owns one (row, frame): the row is read coalesced, binned with LDS atomics, written once, and its maximum goes
 * to a single global atomicMax.  Integer counts and maxima do not depend on the order, so the result is identical. */
__global__ __launch_bounds__(256) void k_road_histogram(const float* __restrict__ disparity,
                                                        int* __restrict__ vdisp, int* __restrict__ counters,
                                                        int rows, int cols, int max_dis) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* bins = (int*)smem; /* [max_dis] */
    const int row = blockIdx.x, f = blockIdx.y;
    for (int i = threadIdx.x; i < max_dis; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const float* src = disparity + ((size_t)f * rows + row) * cols;
    for (int j = threadIdx.x; j < cols; j += blockDim.x) {
        const float d = src[j];
        if (d != 0) {
            /* RoadEstimationKernels.cu:33-37: the bin is (int)d, truncation toward zero.  NaN goes to bin 0,
             * stated here and not left to the conversion: the reference's float -> int of NaN gives 0 on its
             * GPU, in C++ (int)NaN is undefined.  The bin guard (the reference is unchecked) is the float
             * range (-1, max_dis), so +-inf and |d| >= 2^31 are never converted and fall in no bin. */
            if (d != d) atomicAdd(&bins[0], 1);
            else if (d > -1.0f && d < (float)max_dis) atomicAdd(&bins[(int)d], 1);
        }
    }
    __syncthreads();
    int m = 0;
    int* dst = vdisp + ((size_t)f * rows + row) * max_dis;
    for (int i = threadIdx.x; i < max_dis; i += blockDim.x) {
        const int v = bins[i];
        dst[i] = v;
        m = max(m, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&counters[f * IS_ROAD_CNT + IS_ROAD_CNT_MAX], m);
}

/* Binarisation (RoadEstimationKernels.cu:55-58) and, WITH_POINTS, compaction of the non-zero pixels of each
 * frame into points[f][k] = (i << 16) | j (rows <= 32767).  One atomic per wave: the ballot's popcount reserves
 * the wave's slots.  Without it neither the point counter nor `points` is read or written. */
template <bool WITH_POINTS>
__global__ __launch_bounds__(256) void k_road_binarize(const int* __restrict__ vdisp, uint8_t* __restrict__ binary,
                                                       int* __restrict__ counters, int* __restrict__ points,
                                                       float threshold, int rows, int max_dis) {
    const int f = blockIdx.y;
    const int n = rows * max_dis;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t off = (size_t)f * n;
    bool on = false;
    if (idx < n) {
        const float p = (float)vdisp[off + idx];
        on = p > counters[f * IS_ROAD_CNT + IS_ROAD_CNT_MAX] * threshold;
        binary[off + idx] = on ? 255 : 0;
    }
    if (!WITH_POINTS) return;
    const uint64_t mask = __ballot(on);
    if (mask == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&counters[f * IS_ROAD_CNT + IS_ROAD_CNT_POINTS], __popcll(mask));
    base = __shfl(base, leader, 64);
    if (on) {
        const int k = base + __popcll(mask & ((1ull << lane) - 1));
        points[off + k] = ((idx / max_dis) << 16) | (idx % max_dis); /* k < n: one slot per pixel */
    }
}

/* Hough vote + local maxima of one (band of angles, frame).  The band's accumulator rows and one halo row on
 * each side live in LDS: lds[k][numrho + 2] holds accumulator row n0 + k (angle n0 + k - 1), k = 0 .. band + 1.
 * Rows of angles outside [0, numangle) are the accumulator's zero padding; so are the columns 0 and
 * numrho + 1.  Votes: r = rint(j*tabCos[a] + i*tabSin[a]) in fp32 without contraction, as HoughLines. */
__global__ __launch_bounds__(256) void k_road_hough(const int* __restrict__ points,
                                                    const int* __restrict__ counters,
                                                    const float* __restrict__ tab, /* [sin | cos][numangle] */
                                                    int2* __restrict__ cand, int* __restrict__ ncand,
                                                    int n_cells, int numangle, int numrho, int band,
                                                    int threshold, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* acc = (int*)smem;
    const int f = blockIdx.y;
    const int n0 = blockIdx.x * band; /* first angle of the band */
    const int stride = numrho + 2;
    const int lrows = band + 2;
    for (int k = threadIdx.x; k < lrows * stride; k += blockDim.x) acc[k] = 0;
    __syncthreads();
    const int a_lo = max(n0 - 1, 0), a_hi = min(n0 + band + 1, numangle); /* angles voted here */
    const int npts = counters[f * IS_ROAD_CNT + IS_ROAD_CNT_POINTS];
    const int* pts = points + (size_t)f * n_cells;
    const float* tabSin = tab;
    const float* tabCos = tab + numangle;
    const int roff = (numrho - 1) / 2;
    for (int p = threadIdx.x; p < npts; p += blockDim.x) {
        const int v = pts[p];
        const float fi = (float)(v >> 16), fj = (float)(v & 0xffff);
        for (int a = a_lo; a < a_hi; a++) {
            const float x = fj * tabCos[a];
            const float y = fi * tabSin[a];
            const int r = (int)rintf(x + y) + roff;
            if (r >= 0 && r < numrho) atomicAdd(&acc[(a - n0 + 1) * stride + r + 1], 1);
        }
    }
    __syncthreads();
    const int nb = min(band, numangle - n0); /* real angles of the band */
    for (int t = threadIdx.x; t < nb * numrho; t += blockDim.x) {
        const int k = t / numrho + 1, r = t % numrho;
        const int lb = k * stride + r + 1;
        const int v = acc[lb];
        if (v > threshold && v > acc[lb - 1] && v >= acc[lb + 1] && v > acc[lb - stride] &&
            v >= acc[lb + stride]) {
            const int slot = atomicAdd(&ncand[f], 1); /* local maxima found (may exceed cap) */
            if (slot < cap) cand[(size_t)f * cap + slot] = make_int2((n0 + k) * stride + r + 1, v);
        }
    }
}

/* Sort of one frame's candidates (votes descending, accumulator index ascending: unique keys, so the order
 * of arrival does not matter) by a bitonic sort of 64-bit keys in LDS, then the first max_lines lines as
 * HoughLines writes them. */
__global__ __launch_bounds__(256) void k_road_sort(const int2* __restrict__ cand, const int* __restrict__ ncand,
                                                   float* __restrict__ lines, int* __restrict__ votes,
                                                   int* __restrict__ total, int* __restrict__ overflow,
                                                   int cap, int max_lines, int numrho, float rho, float theta) {
    __shared__ unsigned long long keys[IS_ROAD_SORT_MAX];
    const int f = blockIdx.x;
    const int found = ncand[f];
    const int m = min(found, cap);
    int P = 1;
    while (P < m) P <<= 1;
    for (int t = threadIdx.x; t < P; t += blockDim.x) {
        unsigned long long k = ~0ull;
        if (t < m) {
            const int2 c = cand[(size_t)f * cap + t];
            k = ((unsigned long long)(unsigned)(0x7fffffff - c.y) << 32) | (unsigned)c.x;
        }
        keys[t] = k;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < P; t += blockDim.x) {
                const int u = t ^ stride;
                if (u > t) {
                    const unsigned long long a = keys[t], b = keys[u];
                    const bool up = (t & size) == 0;
                    if ((a > b) == up) { keys[t] = b; keys[u] = a; }
                }
            }
            __syncthreads();
        }
    const double scale = 1. / (numrho + 2);
    const int nl = min(m, max_lines);
    for (int t = threadIdx.x; t < nl; t += blockDim.x) {
        const unsigned long long k = keys[t];
        const int idx = (int)(k & 0xffffffffu);
        const int n = (int)floor(idx * scale) - 1;
        const int r = idx - (n + 1) * (numrho + 2) - 1;
        float* l = lines + ((size_t)f * max_lines + t) * 2;
        l[0] = (r - (numrho - 1) * 0.5f) * rho;
        l[1] = 0.0f + n * theta;
        if (votes) votes[(size_t)f * max_lines + t] = 0x7fffffff - (int)(k >> 32);
    }
    if (threadIdx.x == 0) {
        total[f] = found;
        overflow[f] = found > cap ? 1 : 0;
    }
}

/* The line choice of one frame per wave (RoadEstimation::ChooseLineShared, bitwise): the lanes evaluate the lines
 * lane, lane + 64, ... of the sorted list with is_road_line, and the lowest accepted index of a round wins by
 * ballot.  Only lines k < min(total, max_lines) are read: what k_road_sort wrote.  tabT: [sin | cos][numangle] of
 * the transform's angles, the host's sinf / cosf. */
__global__ __launch_bounds__(64) void k_road_choose(const float* __restrict__ lines, const int* __restrict__ total,
                                                    const int* __restrict__ overflow, const float* __restrict__ tabT,
                                                    is_road_params* __restrict__ road, uint8_t* __restrict__ status,
                                                    int max_lines, int numangle, float step, int rows, float cy,
                                                    float baseline, float focal, float min_pitch, float max_pitch,
                                                    is_road_params fallback) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int found = total[f];
    const bool over = overflow[f] != 0;
    const int nl = over ? 0 : min(found, max_lines); /* (an overflowed sort: not HoughLines' lines) */
    const float* fl = lines + (size_t)f * max_lines * 2;
    is_road_params out = fallback;
    int st = over || found > max_lines ? IS_ROAD_UNDECIDED : IS_ROAD_NONE;
    for (int base = 0; base < nl; base += 64) { /* (wave-uniform trip count) */
        const int k = base + lane;
        is_road_params mine = fallback;
        int accepted = 0, vhor_ok = 0;
        if (k < nl) {
            const float rho = fabsf(fl[2 * k]);
            const int n = is_road_angle_index(fl[2 * k + 1], step, numangle);
            if (n >= 0)
                accepted = is_road_line(rho, tabT[n], tabT[numangle + n], cy, baseline, focal, rows, min_pitch,
                                        max_pitch, &mine, &vhor_ok);
        }
        const uint64_t mask = __ballot(accepted);
        if (mask != 0) {
            const int leader = __ffsll((unsigned long long)mask) - 1;
            /* (every lane takes the leader's values: the stores below come from lane 0) */
            const int ok = __shfl(vhor_ok, leader, 64);
            st = ok ? IS_ROAD_OK : IS_ROAD_HORIZON;
            if (ok) {
                out.vhor = __shfl(mine.vhor, leader, 64);
                out.tilt = __shfl(mine.tilt, leader, 64);
                out.height = __shfl(mine.height, leader, 64);
                out.alpha = __shfl(mine.alpha, leader, 64);
            }
            break;
        }
    }
    if (lane == 0) {
        road[f] = out;
        status[f] = (uint8_t)st;
    }
}

extern "C" {

int isk_road_sort_max(void) { return IS_ROAD_SORT_MAX; }
int isk_road_counters(void) { return IS_ROAD_CNT; }

hipError_t isk_set_lds_road_hough(int bytes) {
    return hipFuncSetAttribute((const void*)k_road_hough, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

/* counters [n][IS_ROAD_CNT] must be zero on entry (the caller clears them in one memset) */
hipError_t isk_launch_road_vdisparity(const float* disparity, int* vdisp, uint8_t* binary, int* counters,
                                      int* points, int n_images, int rows, int cols, int max_dis,
                                      float threshold, hipStream_t stream) {
    hipLaunchKernelGGL(k_road_histogram, dim3(rows, n_images), dim3(256), sizeof(int) * max_dis, stream,
                       disparity, vdisp, counters, rows, cols, max_dis);
    const int n = rows * max_dis;
    hipLaunchKernelGGL(k_road_binarize<true>, dim3((n + 255) / 256, n_images), dim3(256), 0, stream, vdisp, binary,
                       counters, points, threshold, rows, max_dis);
    return hipGetLastError();
}

/* One frame without a point list (any rows): *maximum, zero on entry, is frame 0's IS_ROAD_CNT_MAX. */
hipError_t isk_launch_road_vdisparity_single(const float* disparity, int* vdisp, uint8_t* binary, int* maximum,
                                             int rows, int cols, int max_dis, float threshold, hipStream_t stream) {
    static_assert(IS_ROAD_CNT_MAX == 0, "the caller's int is entry 0 of frame 0's counters");
    hipLaunchKernelGGL(k_road_histogram, dim3(rows, 1), dim3(256), sizeof(int) * max_dis, stream, disparity, vdisp,
                       maximum, rows, cols, max_dis);
    const int n = rows * max_dis;
    hipLaunchKernelGGL(k_road_binarize<false>, dim3((n + 255) / 256, 1), dim3(256), 0, stream, vdisp, binary,
                       maximum, nullptr, threshold, rows, max_dis);
    return hipGetLastError();
}

/* ncand [n] must be zero on entry */
hipError_t isk_launch_road_hough(const int* points, const int* counters, int* ncand, const float* tab, int2* cand,
                                 float* lines, int* votes, int* total, int* overflow, int n_images, int n_cells, int numangle,
                                 int numrho, int band, int threshold, int cap, int max_lines, float rho,
                                 float theta, hipStream_t stream) {
    const int nbands = (numangle + band - 1) / band;
    const size_t lds = sizeof(int) * (size_t)(band + 2) * (numrho + 2);
    hipLaunchKernelGGL(k_road_hough, dim3(nbands, n_images), dim3(256), lds, stream, points, counters, tab, cand,
                       ncand, n_cells, numangle, numrho, band, threshold, cap);
    hipLaunchKernelGGL(k_road_sort, dim3(n_images), dim3(256), 0, stream, cand, ncand, lines, votes, total,
                       overflow, cap, max_lines, numrho, rho, theta);
    return hipGetLastError();
}

hipError_t isk_launch_road_choose(const float* lines, const int* total, const int* overflow, const float* tabT,
                                  is_road_params* road, uint8_t* status, int n_images, int max_lines, int numangle,
                                  float step, int rows, float cy, float baseline, float focal, float min_pitch,
                                  float max_pitch, is_road_params fallback, hipStream_t stream) {
    hipLaunchKernelGGL(k_road_choose, dim3(n_images), dim3(64), 0, stream, lines, total, overflow, tabT, road, status,
                       max_lines, numangle, step, rows, cy, baseline, focal, min_pitch, max_pitch, fallback);
    return hipGetLastError();
}

} /* extern "C" */
