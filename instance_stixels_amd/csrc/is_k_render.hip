/*
 * is_k_render.hip -- f5: stixels to dense per-pixel result maps (label, disparity, instance images) and their
 * scores against ground truth (confusion matrix, disparity deviation, stixel count), n frames per launch.
 * The geometry is that of the reference tooling's draw_stixels (see is_render_sections in
 * instance_stixels_core.h); the numpy restatement is tests/render_reference.py.
 *
 * One lane owns one stixel column (w pixels wide) and IS_RENDER_RCH image rows.  It first paints the index of
 * the section that covers each of its rows into a lane-private LDS strip (sections in index order, so the
 * highest index wins where hand-built sections overlap; -1 = uncovered), then walks its rows top-down and writes
 * each row's w pixels.  The 64 lanes of a wave are 64 adjacent stixel columns at the same row, so every store
 * instruction writes one contiguous run of the row: 512 B for the label image, 2 x 1 KiB for the 4-byte images
 * when w == 8.  The images are written once and never read back; the cost is their write bandwidth.
 * Metrics use the pixels already in registers: confusion bins in LDS, one LDS add per run of equal
 * (gt, pred) pairs (within a row and down the rows), non-zero bins flushed with 64-bit global atomics; the
 * disparity deviation in fp64 per lane, reduced in a fixed order to one partial per workgroup, and the partials
 * of a frame summed in a fixed order by k_render_finalize -- the same bits on every run.  The paint loops of
 * the first row group also count each column's sections for the stixel count.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_launch.h"

#define IS_RENDER_RCH 32    /* image rows per lane */
#define IS_RENDER_WAVES 4   /* waves per workgroup, stacked vertically: 128 rows x 64 stixel columns */
#define IS_RENDER_TABLE IS_RENDER_MAX_CLASSES /* the class -> label table travels in the kernel arguments */

struct RenderArgs {
    const is_section* sections;
    const int32_t* section_instance;
    uint8_t* label;
    float* disparity;
    int32_t* instance;
    const uint8_t* gt_label;
    const float* gt_disparity;
    unsigned long long* confusion;
    double* partial_sum;       /* [n][row_groups * col_groups]: deviation sums, NULL without a deviation */
    long long* partial_count;
    int* partial_stixels;      /* [n][col_groups]: sections of the workgroup's columns (row group 0 only) */
    int realcols, max_sections, rows, cols, w, xlanes, row_groups, n_labels, n_classes;
    uint8_t table[IS_RENDER_TABLE];
};

__device__ __forceinline__ void conf_add(unsigned* bins, int& key, unsigned& run, int k) {
    if (k == key) {
        run++;
        return;
    }
    if (run) atomicAdd(&bins[key], run);
    key = k;
    run = 1;
}

/* VEC: w == 8 and every row 8-pixel aligned (cols % 8 == 0, aligned base pointers): vector stores and loads
 * for the stixel columns; the tail lane (pixels right of realcols * w) always takes the per-pixel path. */
template <bool VEC>
__global__ __launch_bounds__(64 * IS_RENDER_WAVES) void k_render(const RenderArgs a) {
    __shared__ int16_t strip[IS_RENDER_WAVES][IS_RENDER_RCH][64];
    __shared__ unsigned bins[IS_RENDER_MAX_LABELS * IS_RENDER_MAX_LABELS];
    __shared__ double red_sum[IS_RENDER_WAVES];
    __shared__ long long red_cnt[IS_RENDER_WAVES];
    __shared__ int red_stixels;
    const int f = blockIdx.x / a.row_groups, rg = blockIdx.x % a.row_groups;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.y * 64 + lane;
    const int y0 = (rg * IS_RENDER_WAVES + wave) * IS_RENDER_RCH;
    const int y1 = min(y0 + IS_RENDER_RCH, a.rows);
    const int nl = a.n_labels;
    const bool conf = a.confusion != nullptr, dev = a.partial_sum != nullptr;
    if (conf)
        for (int i = threadIdx.x; i < nl * nl; i += blockDim.x) bins[i] = 0;
    __syncthreads();

    double dsum = 0;
    long long dcnt = 0;
    int nstix = 0; /* the column's sections in front of its terminator (counted by the paint loop) */
    int key = 0;
    unsigned run = 0;
    if (c < a.xlanes && y0 < y1) {
        int16_t* m = &strip[wave][0][lane];
        for (int r = 0; r < IS_RENDER_RCH; r++) m[r * 64] = -1;
        const bool stixel = c < a.realcols;
        const is_section* col = a.sections + ((size_t)f * a.realcols + (stixel ? c : 0)) * a.max_sections;
        if (stixel)
            for (int i = 0; i < a.max_sections; i++, nstix++) {
                const int4 h = *(const int4*)&col[i]; /* type, vB, vT, disparity */
                if (h.x == -1) break;
                /* rows [rows-1-vT, rows-1-vB] of the image, clipped to this lane's rows (64-bit: hostile vB / vT) */
                const long long top = (long long)a.rows - 1 - h.z, bot = (long long)a.rows - 1 - h.y;
                const long long lo = max(top, (long long)y0), hi = min(bot, (long long)y1 - 1);
                if (lo > hi) continue; /* (checked in 64 bits: then both lie in [y0, y1-1]) */
                for (int y = (int)lo; y <= (int)hi; y++) m[(y - y0) * 64] = (int16_t)i;
            }
        const int x0 = c * a.w;
        const int npx = stixel ? a.w : a.cols - a.realcols * a.w;
        int cur = -2;
        uint8_t lab = 0;
        float dv = 0.f;
        int32_t iv = 0;
        for (int y = y0; y < y1; y++) {
            const int s = m[(y - y0) * 64];
            if (s != cur) {
                cur = s;
                lab = 0; dv = 0.f; iv = 0;
                if (s >= 0) {
                    const is_section& sec = col[s];
                    const int cls = sec.semantic_class;
                    dv = sec.disparity;
                    if (cls >= 0 && cls < a.n_classes) lab = a.table[cls];
                    if (a.section_instance) {
                        const int l = a.section_instance[((size_t)f * a.realcols + c) * a.max_sections + s];
                        if (l >= 0 && l < 1000) iv = (int32_t)((uint32_t)cls * 1000u + (uint32_t)l);
                    }
                }
            }
            const size_t pix = ((size_t)f * a.rows + y) * a.cols + x0;
            if (VEC && stixel) {
                if (a.label) *(uint64_t*)(a.label + pix) = 0x0101010101010101ull * lab;
                if (a.disparity) {
                    const float4 v = make_float4(dv, dv, dv, dv);
                    ((float4*)(a.disparity + pix))[0] = v;
                    ((float4*)(a.disparity + pix))[1] = v;
                }
                if (a.instance) {
                    const int4 v = make_int4(iv, iv, iv, iv);
                    ((int4*)(a.instance + pix))[0] = v;
                    ((int4*)(a.instance + pix))[1] = v;
                }
                if (conf) {
                    const uint64_t g = *(const uint64_t*)(a.gt_label + pix);
                    if (lab < nl)
                        for (int k = 0; k < 8; k++) {
                            const int gt = (int)((g >> (8 * k)) & 255);
                            if (gt < nl) conf_add(bins, key, run, gt * nl + lab);
                        }
                }
                if (dev && dv != 0.f) {
                    const float4 g0 = ((const float4*)(a.gt_disparity + pix))[0];
                    const float4 g1 = ((const float4*)(a.gt_disparity + pix))[1];
                    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
                    for (int k = 0; k < 8; k++)
                        if (g[k] != 0.f) {
                            dsum += (double)fabsf(dv - g[k]);
                            dcnt++;
                        }
                }
            } else {
                for (int k = 0; k < npx; k++) {
                    if (a.label) a.label[pix + k] = lab;
                    if (a.disparity) a.disparity[pix + k] = dv;
                    if (a.instance) a.instance[pix + k] = iv;
                    if (conf && lab < nl) {
                        const int gt = a.gt_label[pix + k];
                        if (gt < nl) conf_add(bins, key, run, gt * nl + lab);
                    }
                    if (dev && dv != 0.f) {
                        const float g = a.gt_disparity[pix + k];
                        if (g != 0.f) {
                            dsum += (double)fabsf(dv - g);
                            dcnt++;
                        }
                    }
                }
            }
        }
    }
    if (conf && run) atomicAdd(&bins[key], run);
    if (a.partial_stixels && rg == 0 && wave == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nstix += __shfl_xor(nstix, o, 64);
        if (lane == 0) red_stixels = nstix;
    }
    if (dev) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            dsum += __shfl_xor(dsum, o, 64);
            dcnt += __shfl_xor(dcnt, o, 64);
        }
        if (lane == 0) {
            red_sum[wave] = dsum;
            red_cnt[wave] = dcnt;
        }
    }
    __syncthreads();
    if (dev && threadIdx.x == 0) {
        double s = 0;
        long long n = 0;
        for (int i = 0; i < IS_RENDER_WAVES; i++) {
            s += red_sum[i];
            n += red_cnt[i];
        }
        const size_t p = (size_t)f * a.row_groups * gridDim.y + (size_t)rg * gridDim.y + blockIdx.y;
        a.partial_sum[p] = s;
        a.partial_count[p] = n;
    }
    if (a.partial_stixels && rg == 0 && threadIdx.x == 0)
        a.partial_stixels[(size_t)f * gridDim.y + blockIdx.y] = red_stixels;
    if (conf)
        for (int i = threadIdx.x; i < nl * nl; i += blockDim.x)
            if (bins[i]) atomicAdd(&a.confusion[i], (unsigned long long)bins[i]);
}

/* One lane per frame: the stixel count and the deviation of the frame from the partials of its workgroups,
 * summed in index order. */
__global__ __launch_bounds__(64) void k_render_finalize(const double* __restrict__ partial_sum,
                                                        const long long* __restrict__ partial_count, int parts,
                                                        const int* __restrict__ partial_stixels, int col_groups,
                                                        int n, double* disp_sum, int64_t* disp_count,
                                                        int32_t* stixel_count) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    if (stixel_count) {
        int k = 0;
        for (int i = 0; i < col_groups; i++) k += partial_stixels[(size_t)f * col_groups + i];
        stixel_count[f] = k;
    }
    if (disp_sum) {
        double s = 0;
        long long c = 0;
        for (int i = 0; i < parts; i++) {
            s += partial_sum[(size_t)f * parts + i];
            c += partial_count[(size_t)f * parts + i];
        }
        disp_sum[f] = s;
        disp_count[f] = c;
    }
}

/* The per-candidate cluster labels of up to IS_RENDER_SCATTER_IMAGES frames into the per-section map. */
#define IS_RENDER_SCATTER_IMAGES 64
struct ScatterArgs {
    const int32_t* indices[IS_RENDER_SCATTER_IMAGES];
    const int32_t* labels[IS_RENDER_SCATTER_IMAGES];
    const int32_t* per_class[IS_RENDER_SCATTER_IMAGES];
};

__global__ __launch_bounds__(256) void k_section_instance(const ScatterArgs s, int32_t* __restrict__ out,
                                                          int first_image, int realcols, int max_sections) {
    const int cls = blockIdx.x, i = blockIdx.y;
    const int cs = realcols * max_sections;
    const int n = min(max(s.per_class[i][cls], 0), cs);
    const int32_t* idx = s.indices[i] + (size_t)cls * cs * 2;
    const int32_t* lab = s.labels[i] + (size_t)cls * cs;
    int32_t* dst = out + (size_t)(first_image + i) * cs;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int u = idx[2 * j], v = idx[2 * j + 1];
        if (u >= 0 && u < realcols && v >= 0 && v < max_sections) dst[(size_t)u * max_sections + v] = lab[j];
    }
}

extern "C" {

int isk_render_scatter_images(void) { return IS_RENDER_SCATTER_IMAGES; }

/* out [n][realcols][max_sections] must hold -1 on entry; per_image: n_images (<= IS_RENDER_SCATTER_IMAGES) */
hipError_t isk_launch_section_instance(const is_instance_buffers* per_image, int n_images, int first_image,
                                       int realcols, int max_sections, int32_t* out, hipStream_t stream) {
    ScatterArgs s = {};
    for (int i = 0; i < n_images; i++) {
        s.indices[i] = per_image[i].d_indices;
        s.labels[i] = per_image[i].d_labels;
        s.per_class[i] = per_image[i].d_instances_per_class;
    }
    hipLaunchKernelGGL(k_section_instance, dim3(IS_INSTANCE_CLASSES, n_images), dim3(256), 0, stream, s, out,
                       first_image, realcols, max_sections);
    return hipGetLastError();
}

/* The arguments are checked by is_render_sections.  table: IS_RENDER_TABLE entries (classes >= n_classes are 0). */
hipError_t isk_launch_render(const is_render_args* r, const uint8_t* table, int n_classes, hipStream_t stream) {
    RenderArgs a = {};
    a.sections = r->d_sections;
    a.section_instance = r->d_section_instance;
    a.label = r->d_label;
    a.disparity = r->d_disparity;
    a.instance = r->d_instance;
    a.gt_label = r->d_gt_label;
    a.gt_disparity = r->d_gt_disparity;
    a.confusion = r->d_confusion;
    a.realcols = r->realcols;
    a.max_sections = r->max_sections;
    a.rows = r->rows;
    a.cols = r->cols;
    a.w = r->cols / r->realcols;
    a.xlanes = r->realcols + (r->cols > r->realcols * a.w ? 1 : 0);
    a.row_groups = (r->rows + IS_RENDER_RCH * IS_RENDER_WAVES - 1) / (IS_RENDER_RCH * IS_RENDER_WAVES);
    a.n_labels = r->d_confusion ? r->n_labels : 1;
    a.n_classes = n_classes;
    for (int i = 0; i < IS_RENDER_TABLE; i++) a.table[i] = table[i];
    const int col_groups = (a.xlanes + 63) / 64;
    const int parts = a.row_groups * col_groups;
    const int n = r->n_images;
    const bool dev = r->d_disp_abs_sum != nullptr, cnt = r->d_stixel_count != nullptr;
    void* scratch = nullptr;
    if (dev || cnt) {
        const size_t bytes = (size_t)n * parts * (sizeof(double) + sizeof(long long)) + (size_t)n * col_groups * sizeof(int);
        const hipError_t e = hipMallocAsync(&scratch, bytes, stream);
        if (e != hipSuccess) return e;
        if (dev) {
            a.partial_sum = (double*)scratch;
            a.partial_count = (long long*)(a.partial_sum + (size_t)n * parts);
        }
        if (cnt) a.partial_stixels = (int*)((char*)scratch + (size_t)n * parts * (sizeof(double) + sizeof(long long)));
    }
    /* rows 8-pixel aligned, w == 8, vector-aligned bases: the vector path */
    const uintptr_t al = (uintptr_t)a.label | (uintptr_t)a.gt_label;
    const uintptr_t a16 = (uintptr_t)a.disparity | (uintptr_t)a.instance | (uintptr_t)a.gt_disparity;
    const bool vec = a.w == 8 && a.cols % 8 == 0 && (al & 7) == 0 && (a16 & 15) == 0;
    const bool work = a.label || a.disparity || a.instance || a.confusion || dev || cnt;
    if (work) {
        const dim3 grid((unsigned)(n * a.row_groups), (unsigned)col_groups);
        if (vec)
            hipLaunchKernelGGL(k_render<true>, grid, dim3(64 * IS_RENDER_WAVES), 0, stream, a);
        else
            hipLaunchKernelGGL(k_render<false>, grid, dim3(64 * IS_RENDER_WAVES), 0, stream, a);
    }
    if (dev || cnt)
        hipLaunchKernelGGL(k_render_finalize, dim3((n + 63) / 64), dim3(64), 0, stream, a.partial_sum,
                           a.partial_count, parts, a.partial_stixels, col_groups, n, r->d_disp_abs_sum,
                           r->d_disp_count, r->d_stixel_count);
    hipError_t e = hipGetLastError();
    if (scratch) {
        const hipError_t e2 = hipFreeAsync(scratch, stream);
        if (e == hipSuccess) e = e2;
    }
    return e;
}

} /* extern "C" */
