/*
 * is_k_cnn_labels.hip -- f15: the CNN's own label image of a batch at full resolution and its confusion table, from
 * the 1/8-resolution cost planes of f13, in one launch (is_cnn_label_maps in instance_stixels_core.h; the C loop
 * of tests/cnn_labels_reference.py is the contract restated).
 *
 * A workgroup owns IS_CNN_TH x IS_CNN_TW cells, 64 x 256 pixels.  It stages the n_classes values of those cells and
 * of a one-cell halo in LDS (cnn_up_stage in is_cnn_up.h: a cell outside the plane is the contract's skipped tap).
 * One lane owns one cell: 8 image rows of 8 pixels.  The 8 pixels of a row read 3 x 2 cells per class (pixels 0..3
 * the cells left and centre, 4..7 centre and right; rows 0..3 the cells above and centre, 4..7 centre and below),
 * so a class costs 6 LDS reads and 32 fmaf per row, and no upsampled value is ever stored.  The 32 lanes of a half
 * wave are 32 adjacent cells: every store instruction writes 256 contiguous bytes of two image rows.  The nearest
 * mode is the same kernel with the cell's own class in all 64 pixels.
 * Confusion bins in LDS as in is_k_render.hip: one LDS add per run of equal (gt, pred) pairs (8 pixels whose bytes
 * are all equal extend the run in one step), non-zero bins flushed with 64-bit integer atomics.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_cnn_up.h"
#include "is_launch.h"

#define IS_CNN_TW 32                                   /* cells per tile row: one half wave */
#define IS_CNN_TH 8                                    /* cell rows per tile */
#define IS_CNN_PITCH (IS_CNN_TW + 2)
#define IS_CNN_CELLS ((IS_CNN_TH + 2) * IS_CNN_PITCH)  /* one class of a tile with its halo */

struct CnnLabelArgs {
    const float* cnn;
    uint8_t* class8;
    uint8_t* label;
    const uint8_t* gt;
    unsigned long long* confusion;
    int channels, n_classes, rows8, cols8, cols, xcells, xtiles, n_labels;
    uint8_t table[IS_HEAD_MAX_CHANNELS];
};

/* n more pixels of bin k: a lane keeps the run of its current bin in registers and adds it to LDS when the bin
 * changes */
__device__ __forceinline__ void cnn_conf_add(unsigned* bins, int& key, unsigned& run, int k, unsigned n) {
    if (k == key) {
        run += n;
        return;
    }
    if (run) atomicAdd(&bins[key], run);
    key = k;
    run = n;
}

/* DECONV: IS_CNN_UP_DECONV, else IS_CNN_UP_NEAREST.  VEC: cols % 8 == 0 and 8-byte aligned label images, so that a
 * lane's 8 pixels of a row are one 64-bit access; else byte by byte. */
template <bool DECONV, bool VEC>
__global__ __launch_bounds__(256) void k_cnn_labels(const CnnLabelArgs a) {
    extern __shared__ __align__(16) unsigned char cnn_lds[];
    const int ncls = a.n_classes, nl = a.n_labels;
    float* tile = (float*)cnn_lds;                         /* [ncls][IS_CNN_TH + 2][IS_CNN_PITCH] */
    unsigned* bins = (unsigned*)(tile + ncls * IS_CNN_CELLS); /* [nl][nl] */
    uint8_t* table = (uint8_t*)(bins + nl * nl);           /* [IS_HEAD_MAX_CHANNELS] */
    const int f = blockIdx.y;
    const int ty0 = (blockIdx.x / a.xtiles) * IS_CNN_TH, tx0 = (blockIdx.x % a.xtiles) * IS_CNN_TW;
    const int tid = threadIdx.x;
    const bool conf = a.confusion != nullptr;
    const int P = a.rows8 * a.cols8;

    if (tid < IS_HEAD_MAX_CHANNELS) table[tid] = a.table[tid];
    if (conf)
        for (int i = tid; i < nl * nl; i += 256) bins[i] = 0;
    if (tx0 < a.cols8) /* (a tile of margin cells alone reads nothing) */
        cnn_up_stage<IS_CNN_TH + 2, IS_CNN_PITCH, 256>(tile, a.cnn + (size_t)f * a.channels * P, ncls, ty0 - 1, tx0 - 1,
                                                        a.rows8, a.cols8, tid);
    __syncthreads();

    const int lx = tid & (IS_CNN_TW - 1), ly = tid / IS_CNN_TW;
    const int c = tx0 + lx, cy = ty0 + ly;
    const bool cell = cy < a.rows8 && c < a.cols8;      /* a cell of the plane */
    const bool margin = cy < a.rows8 && !cell && c < a.xcells; /* pixels right of the plane: label 0 */
    int key = 0;
    unsigned run = 0;
    if (cell || margin) {
        const float* t0 = tile + (ly + 1) * IS_CNN_PITCH + (lx + 1);
        int own = 0;
        if (cell) {
            float best = t0[0];
            for (int k = 1; k < ncls; k++) {
                const float v = t0[k * IS_CNN_CELLS];
                if (v < best) {
                    best = v;
                    own = k;
                }
            }
            if (a.class8) a.class8[(size_t)f * P + cy * a.cols8 + c] = (uint8_t)own;
        }
        if (a.label || conf) {
            const int npx = cell ? 8 : min(8, a.cols - 8 * c);
            const size_t pix0 = ((size_t)f * (8 * a.rows8) + 8 * cy) * a.cols + 8 * c;
            /* the ground truth of the lane's 8 rows, requested at once: 8 loads in flight, not one after the other */
            uint64_t g8[8] = {};
            if (VEC && conf && cell) {
#pragma unroll
                for (int j = 0; j < 8; j++) g8[j] = *(const uint64_t*)(a.gt + pix0 + (size_t)j * a.cols);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                int idx[8];
                if (DECONV && cell) {
                    /* rows 0..3 of the cell: r = j + 4, the cells above and centre; rows 4..7: r = j - 4, centre
                     * and below.  The same for the pixels of the row with the cells left, centre and right. */
                    const int rj = (j + 4) & 7;
                    const float* p = t0 + (j < 4 ? -IS_CNN_PITCH : 0);
                    float w[8][4];
                    cnn_up_weights(w, cnn_w_low(rj), cnn_w_high(rj), 4);
                    float best[8];
                    for (int cls = 0; cls < ncls; cls++, p += IS_CNN_CELLS) {
                        const float u[3] = {p[-1], p[0], p[1]};
                        const float d[3] = {p[IS_CNN_PITCH - 1], p[IS_CNN_PITCH], p[IS_CNN_PITCH + 1]};
#pragma unroll
                        for (int k = 0; k < 8; k++) {
                            const int x = k < 4 ? 0 : 1;
                            const float acc = cnn_up_chain(w[k], u[x], u[x + 1], d[x], d[x + 1]);
                            if (cls == 0) {
                                best[k] = acc;
                                idx[k] = 0;
                            } else if (acc < best[k]) {
                                best[k] = acc;
                                idx[k] = cls;
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++) idx[k] = own;
                }
                uint8_t lab[8];
#pragma unroll
                for (int k = 0; k < 8; k++) lab[k] = cell ? table[idx[k]] : (uint8_t)0;
                const size_t pix = pix0 + (size_t)j * a.cols;
                if (VEC) {
                    uint64_t v = 0;
#pragma unroll
                    for (int k = 0; k < 8; k++) v |= (uint64_t)lab[k] << (8 * k);
                    if (a.label) *(uint64_t*)(a.label + pix) = v;
                    if (conf && cell) {
                        const uint64_t g = g8[j];
                        if (g == ((g << 8) | (g >> 56)) && v == ((v << 8) | (v >> 56))) {
                            /* 8 equal bytes in both (label images are mostly so): one pair, counted 8 times */
                            if ((int)(g & 255) < nl && lab[0] < nl)
                                cnn_conf_add(bins, key, run, (int)(g & 255) * nl + lab[0], 8);
                        } else {
#pragma unroll
                            for (int k = 0; k < 8; k++) {
                                const int gt = (int)((g >> (8 * k)) & 255);
                                if (gt < nl && lab[k] < nl) cnn_conf_add(bins, key, run, gt * nl + lab[k], 1);
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        if (k >= npx) break;
                        if (a.label) a.label[pix + k] = lab[k];
                        if (conf && cell) {
                            const int gt = a.gt[pix + k];
                            if (gt < nl && lab[k] < nl) cnn_conf_add(bins, key, run, gt * nl + lab[k], 1);
                        }
                    }
                }
            }
        }
    }
    if (conf) {
        if (run) atomicAdd(&bins[key], run);
        __syncthreads();
        for (int i = tid; i < nl * nl; i += 256)
            if (bins[i]) atomicAdd(&a.confusion[i], (unsigned long long)bins[i]);
    }
}

extern "C" {

/* The arguments are checked by is_cnn_label_maps.  table: IS_HEAD_MAX_CHANNELS entries (classes outside the caller's
 * table are 0). */
hipError_t isk_launch_cnn_labels(const is_cnn_label_args* r, const uint8_t* table, hipStream_t stream) {
    CnnLabelArgs a = {};
    a.cnn = r->d_cnn_out;
    a.class8 = r->d_class8;
    a.label = r->d_label;
    a.gt = r->d_gt_label;
    a.confusion = r->d_confusion;
    a.channels = r->channels;
    a.n_classes = r->n_classes;
    a.rows8 = r->rows8;
    a.cols8 = r->cols8;
    a.cols = r->cols;
    /* without an image only the plane's cells are visited; with one, the cells of the margin too */
    a.xcells = (a.label || a.confusion) ? (r->cols + 7) / 8 : r->cols8;
    a.xtiles = (a.xcells + IS_CNN_TW - 1) / IS_CNN_TW;
    a.n_labels = r->d_confusion ? r->n_labels : 0;
    for (int i = 0; i < IS_HEAD_MAX_CHANNELS; i++) a.table[i] = table[i];
    const int ytiles = (r->rows8 + IS_CNN_TH - 1) / IS_CNN_TH;
    const size_t lds = sizeof(float) * a.n_classes * IS_CNN_CELLS + sizeof(unsigned) * a.n_labels * a.n_labels +
                       IS_HEAD_MAX_CHANNELS;
    const dim3 grid((unsigned)(a.xtiles * ytiles), (unsigned)r->n_images);
    const bool vec = r->cols % 8 == 0 && (((uintptr_t)a.label | (uintptr_t)a.gt) & 7) == 0;
    const bool deconv = r->mode == IS_CNN_UP_DECONV;
    if (deconv && vec)
        hipLaunchKernelGGL((k_cnn_labels<true, true>), grid, dim3(256), lds, stream, a);
    else if (deconv)
        hipLaunchKernelGGL((k_cnn_labels<true, false>), grid, dim3(256), lds, stream, a);
    else if (vec)
        hipLaunchKernelGGL((k_cnn_labels<false, true>), grid, dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL((k_cnn_labels<false, false>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

} /* extern "C" */
