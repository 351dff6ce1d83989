/*
 * is_k_nll_up.hip -- f16: the classification loss of the reference's full-resolution models on f13's cost planes,
 * NLLLoss(mean, ignore_index)(log_softmax(up(.))) with its gradient with respect to the planes, without ever storing
 * an upsampled value (is_semantic_nll_up in instance_stixels_core.h; tests/nll_up_reference.py is the contract
 * restated).
 *
 * The unit of work is a CORNER BLOCK (a, b), a in 0..rows8, b in 0..cols8: the 8 x 8 pixels Y = 8a-4+j, X = 8b-4+k.
 * All 64 have the same four taps, the cells (a-1, b-1), (a-1, b), (a, b-1), (a, b), with the 1-D weights
 * cnn_w_low(j) / cnn_w_high(j) and cnn_w_low(k) / cnn_w_high(k); and these four cells are the only ones their
 * residuals reach.  So a lane that owns one corner block reads four values per class, keeps one float per pixel
 * (K = m - log S, from which p_c = exp(K - u_c)) and reduces the block to four partial sums per class, separably: a
 * row's 8 residuals to two horizontal sums, the 8 rows' to 2 x 2 vertical ones.  A cell is the sum of one partial of
 * each of the four corner blocks around it, added in a fixed order through LDS.
 * A workgroup is NU_TH x NU_TW corner blocks, one per lane, and writes the (NU_TH - 1) x (NU_TW - 1) cells between
 * them: the last block row and column of a tile are computed again by the next tile (1.18 x the arithmetic, no
 * hand-over through memory and no atomics).  The loss and the counts of a block are taken by exactly one tile.
 * Cells outside the plane are staged as +0.0f, the contract's skipped tap (cnn_up_stage in is_cnn_up.h).
 * A pixel outside the image, with an ignored target or in a row half that is outside has K = -inf and a target byte
 * of 255: p = 0, no one-hot, residual +0.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_cnn_up.h"
#include "is_launch.h"
#include "is_nll.h"

#define NU_TW 32                                       /* corner blocks per tile row: one half wave */
#define NU_TH 8                                        /* corner block rows per tile */
#define NU_PITCH (NU_TW + 1)                           /* cells tx0 - 1 .. tx0 + NU_TW - 1 */
#define NU_CELLS ((NU_TH + 1) * NU_PITCH)              /* one class of a tile */
#define NU_THREADS (NU_TW * NU_TH)
static_assert(NU_THREADS == NLL_THREADS, "one corner block per thread of nll_tree");
#define NU_SCALE_ITEMS 4                               /* elements per thread of the scaling launch */

struct NllUpArgs {
    const float* cnn;
    long long cnn_stride;
    const uint8_t* target;
    float* grad;
    long long grad_stride;
    nll_partial* partials;
    int n_classes, rows8, cols8, cols, xtiles, ignore;
};

/* GRAD: the gradient is written (unscaled; k_nll_up_scale multiplies by 1 / V).  VEC: cols % 4 == 0 and a 4-byte
 * aligned target, so that the 4 pixels of a block's row half are one 32-bit load; else byte by byte. */
template <bool GRAD, bool VEC>
__global__ __launch_bounds__(NU_THREADS) void k_nll_up(const NllUpArgs a) {
    extern __shared__ __align__(16) unsigned char nu_lds[];
    const int ncls = a.n_classes;
    double* sd = (double*)nu_lds;                          /* [NU_THREADS] */
    int* sv = (int*)(sd + NU_THREADS);                     /* [NU_THREADS] */
    int* sb = sv + NU_THREADS;                             /* [NU_THREADS] */
    float* tile = (float*)(sb + NU_THREADS);               /* [ncls][NU_TH + 1][NU_PITCH] */
    float* xch = tile + ncls * NU_CELLS;                   /* GRAD: [2][4][NU_THREADS] */
    const int f = blockIdx.y;
    const int ty0 = (blockIdx.x / a.xtiles) * (NU_TH - 1), tx0 = (blockIdx.x % a.xtiles) * (NU_TW - 1);
    const int tid = threadIdx.x;
    const int P = a.rows8 * a.cols8;

    cnn_up_stage<NU_TH + 1, NU_PITCH, NU_THREADS>(tile, a.cnn + (long long)f * a.cnn_stride, ncls, ty0 - 1, tx0 - 1,
                                                  a.rows8, a.cols8, tid);
    __syncthreads();

    const int lx = tid & (NU_TW - 1), ly = tid / NU_TW;
    const int ba = ty0 + ly, bb = tx0 + lx;                 /* the lane's corner block */
    const bool exists = ba <= a.rows8 && bb <= a.cols8;
    /* the one tile that takes the block's loss and counts: the last row / column of a tile belongs to the next tile,
     * unless it is the plane's last */
    const bool owner = exists && (ly < NU_TH - 1 || ba == a.rows8) && (lx < NU_TW - 1 || bb == a.cols8);
    const bool active = GRAD ? exists : owner;
    const bool top = ba >= 1, bottom = ba < a.rows8, left = bb >= 1, right = bb < a.cols8;
    const float* t0 = tile + ly * NU_PITCH + lx;            /* cell (ba - 1, bb - 1) of class 0 */

    float K[8][8];
    uint32_t tg[8][2];                                      /* the targets of the pixels that count, else 255 */
    double lsum = 0.0;
    int nvalid = 0, nbad = 0;
    if (active) {
        const long long pix0 = ((long long)f * (8 * a.rows8) + (8 * ba - 4)) * a.cols + (8 * bb - 4);
        uint32_t raw[8][2];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool rowin = j < 4 ? top : bottom;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                uint32_t v = 0xffffffffu;
                if (rowin && (h ? right : left)) {
                    const uint8_t* p = a.target + (pix0 + (long long)j * a.cols + 4 * h);
                    if (VEC)
                        v = *(const uint32_t*)p;
                    else
                        v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
                }
                raw[j][h] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool rowin = j < 4 ? top : bottom;
            tg[j][0] = tg[j][1] = 0xffffffffu;
#pragma unroll
            for (int k = 0; k < 8; k++) K[j][k] = -INFINITY;
            if (rowin) {
                float w[8][4];
                cnn_up_weights(w, cnn_w_low(j), cnn_w_high(j), 0);
                float m[8], S[8];
#pragma unroll
                for (int k = 0; k < 8; k++) m[k] = INFINITY;
                const float* p = t0;
                for (int cls = 0; cls < ncls; cls++, p += NU_CELLS) {
                    const float v00 = p[0], v01 = p[1], v10 = p[NU_PITCH], v11 = p[NU_PITCH + 1];
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const float u = cnn_up_chain(w[k], v00, v01, v10, v11);
                        m[k] = u < m[k] ? u : m[k];
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; k++) S[k] = 0.0f;
                p = t0;
                for (int cls = 0; cls < ncls; cls++, p += NU_CELLS) {
                    const float v00 = p[0], v01 = p[1], v10 = p[NU_PITCH], v11 = p[NU_PITCH + 1];
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const float u = cnn_up_chain(w[k], v00, v01, v10, v11);
                        S[k] += expf(m[k] - u);
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const bool in = k < 4 ? left : right;
                    const int t = (int)((raw[j][k >> 2] >> (8 * (k & 3))) & 255u);
                    const bool cls = in && t < ncls && t != a.ignore;
                    if (owner && in && !cls && t != a.ignore) ++nbad;
                    if (cls) {
                        const float Kv = m[k] - logf(S[k]);
                        const float* q = t0 + t * NU_CELLS; /* (inside the tile: t < ncls) */
                        const float ut = cnn_up_chain(w[k], q[0], q[1], q[NU_PITCH], q[NU_PITCH + 1]);
                        if (owner) {
                            lsum += (double)(ut - Kv);
                            ++nvalid;
                        }
                        K[j][k] = Kv;
                        tg[j][k >> 2] = (tg[j][k >> 2] & ~(255u << (8 * (k & 3)))) | (uint32_t)t << (8 * (k & 3));
                    }
                }
            }
        }
    }

    if (GRAD) {
        const bool outcell = ly < NU_TH - 1 && lx < NU_TW - 1 && ba < a.rows8 && bb < a.cols8;
        float* gout = a.grad + (long long)f * a.grad_stride + ba * a.cols8 + bb;
        const float* p = t0;
        for (int cls = 0; cls < ncls; cls++, p += NU_CELLS) {
            float* x = xch + (cls & 1) * 4 * NU_THREADS;
            if (active) {
                const float v00 = p[0], v01 = p[1], v10 = p[NU_PITCH], v11 = p[NU_PITCH + 1];
                float G00 = 0.0f, G01 = 0.0f, G10 = 0.0f, G11 = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if (j < 4 ? top : bottom) {
                        const float wyl = cnn_w_low(j), wyh = cnn_w_high(j);
                        float hl = 0.0f, hh = 0.0f;
#pragma unroll
                        for (int k = 0; k < 8; k++) {
                            const float wxl = cnn_w_low(k), wxh = cnn_w_high(k);
                            const float w[4] = {wyl * wxl, wyl * wxh, wyh * wxl, wyh * wxh};
                            const float u = cnn_up_chain(w, v00, v01, v10, v11);
                            const float pr = expf(K[j][k] - u);
                            const int t = (int)((tg[j][k >> 2] >> (8 * (k & 3))) & 255u);
                            const float r = (t == cls ? 1.0f : 0.0f) - pr;
                            hl = fmaf(wxl, r, hl);
                            hh = fmaf(wxh, r, hh);
                        }
                        G00 = fmaf(wyl, hl, G00);
                        G01 = fmaf(wyl, hh, G01);
                        G10 = fmaf(wyh, hl, G10);
                        G11 = fmaf(wyh, hh, G11);
                    }
                }
                x[0 * NU_THREADS + tid] = G00;
                x[1 * NU_THREADS + tid] = G01;
                x[2 * NU_THREADS + tid] = G10;
                x[3 * NU_THREADS + tid] = G11;
            }
            /* one barrier per class: the buffer of class c is written again by class c + 2, behind the barrier of
             * class c + 1, which every lane reaches after its reads of class c */
            __syncthreads();
            if (outcell) {
                /* the cell's own block, the one right of it, the one below, the one below right */
                float g = x[3 * NU_THREADS + tid] + x[2 * NU_THREADS + tid + 1];
                g += x[1 * NU_THREADS + tid + NU_TW];
                g += x[0 * NU_THREADS + tid + NU_TW + 1];
                gout[(size_t)cls * P] = g;
            }
        }
    }

    nll_tree(lsum, nvalid, nbad, sd, sv, sb, tid);
    if (tid == 0) a.partials[(size_t)f * gridDim.x + blockIdx.x] = nll_partial{lsum, nvalid, nbad};
}

/* One workgroup.  A frame's records are summed by one wave: lane l takes records l, l + 64, .. in increasing order,
 * the 64 lane sums are folded in halves; a wave adds its frames w, w + 4, .. in increasing order and the four wave
 * sums are added as (0 + 1) + (2 + 3).  So equal frames give equal frame sums, whatever the batch. */
__global__ __launch_bounds__(256) void k_nll_up_final(const nll_partial* __restrict__ in, int n_images, int tiles,
                                                      float* __restrict__ loss, long long* __restrict__ valid,
                                                      long long* __restrict__ bad) {
    __shared__ double sd[256];
    __shared__ long long sv[256], sb[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double total = 0.0;                                    /* (lane 0's is the wave's) */
    long long v = 0, b = 0;
    for (int i = wave; i < n_images; i += 4) {
        const nll_partial* rec = in + (size_t)i * tiles;
        double s = 0.0;
        for (int k = lane; k < tiles; k += 64) s += rec[k].sum, v += rec[k].valid, b += rec[k].bad;
        for (int step = 32; step > 0; step >>= 1) s += __shfl_down(s, step, 64);
        total += s;
    }
    sd[tid] = total, sv[tid] = v, sb[tid] = b;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) sv[tid] += sv[tid + step], sb[tid] += sb[tid + step];
        __syncthreads();
    }
    if (tid == 0) {
        const double s = (sd[0] + sd[64]) + (sd[128] + sd[192]);
        *loss = (float)(s / (double)sv[0]); /* 0 / 0 = NaN without a valid pixel, as torch */
        *valid = sv[0];
        *bad = sb[0];
    }
}

/* grad *= (float)(1.0 / V), one rounding per element; with V = 0 every element is +-0 already and stays so */
__global__ __launch_bounds__(256) void k_nll_up_scale(float* __restrict__ grad, long long grad_stride, int planes,
                                                      const long long* __restrict__ valid) {
    const long long V = *valid;
    const float unit = V > 0 ? (float)(1.0 / (double)V) : 0.0f;
    float* g = grad + (long long)blockIdx.y * grad_stride;
    const long long e0 = (long long)blockIdx.x * (256 * NU_SCALE_ITEMS) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < NU_SCALE_ITEMS; k++) {
        const long long e = e0 + k * 256;
        if (e < planes) g[e] *= unit;
    }
}

static void nll_up_tiles(int rows8, int cols8, int* xtiles, int* ytiles) {
    *xtiles = (cols8 + NU_TW - 2) / (NU_TW - 1);
    *ytiles = (rows8 + NU_TH - 2) / (NU_TH - 1);
}

static size_t nll_up_lds_bytes(int n_classes, bool grad) {
    return NU_THREADS * (sizeof(double) + 2 * sizeof(int)) + sizeof(float) * n_classes * NU_CELLS +
           (grad ? sizeof(float) * 2 * 4 * NU_THREADS : 0);
}

extern "C" size_t isk_semantic_nll_up_scratch_bytes(int n_images, int rows8, int cols8) {
    int xtiles, ytiles;
    nll_up_tiles(rows8, cols8, &xtiles, &ytiles);
    return (size_t)n_images * xtiles * ytiles * sizeof(nll_partial);
}

/* The arguments are checked by is_semantic_nll_up (in-frame offsets fit 31 bits, n_images fits the grid). */
extern "C" hipError_t isk_launch_semantic_nll_up(const is_semantic_nll_up_args* r, hipStream_t stream) {
    NllUpArgs a = {};
    a.cnn = r->d_cnn_out;
    a.cnn_stride = r->cnn_image_stride;
    a.target = r->d_target;
    a.grad = r->d_grad;
    a.grad_stride = r->grad_image_stride;
    a.partials = (nll_partial*)r->d_scratch;
    a.n_classes = r->n_classes;
    a.rows8 = r->rows8;
    a.cols8 = r->cols8;
    a.cols = r->cols;
    a.ignore = r->ignore_index;
    int ytiles;
    nll_up_tiles(r->rows8, r->cols8, &a.xtiles, &ytiles);
    const int tiles = a.xtiles * ytiles;
    const dim3 grid((unsigned)tiles, (unsigned)r->n_images);
    const bool grad = r->d_grad != nullptr;
    const bool vec = r->cols % 4 == 0 && ((uintptr_t)r->d_target & 3) == 0;
    const size_t lds = nll_up_lds_bytes(r->n_classes, grad);
    if (grad && vec)
        hipLaunchKernelGGL((k_nll_up<true, true>), grid, dim3(NU_THREADS), lds, stream, a);
    else if (grad)
        hipLaunchKernelGGL((k_nll_up<true, false>), grid, dim3(NU_THREADS), lds, stream, a);
    else if (vec)
        hipLaunchKernelGGL((k_nll_up<false, true>), grid, dim3(NU_THREADS), lds, stream, a);
    else
        hipLaunchKernelGGL((k_nll_up<false, false>), grid, dim3(NU_THREADS), lds, stream, a);
    hipLaunchKernelGGL(k_nll_up_final, dim3(1), dim3(256), 0, stream, (const nll_partial*)a.partials, r->n_images,
                       tiles, r->d_loss, (long long*)r->d_valid_count, (long long*)r->d_bad_count);
    if (grad) {
        const int planes = r->n_classes * r->rows8 * r->cols8;
        const unsigned blocks = (unsigned)(((long long)planes + 256 * NU_SCALE_ITEMS - 1) / (256 * NU_SCALE_ITEMS));
        hipLaunchKernelGGL(k_nll_up_scale, dim3(blocks, (unsigned)r->n_images), dim3(256), 0, stream, r->d_grad,
                           r->grad_image_stride, planes, (const long long*)r->d_valid_count);
    }
    return hipGetLastError();
}
