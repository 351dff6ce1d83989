/*
 * is_k_nll.hip -- f14: the semantic NLL loss at 1/8 resolution with its gradient (is_semantic_nll).  The contract is
 * the header's section f14.
 *
 * The sum in binary64 over a number of blocks, and ranges per block, that the shape alone decides; a thread adds its
 * pixels in increasing order, a tree in LDS joins the threads (is_nll.h), one block joins the blocks.
 */
#include "is_launch.h"
#include "is_nll.h"

#define NLL_MAX_BLOCKS 1024

/* the blocks of a shape and the pixels (a multiple of the block size) of each */
static void nll_plan(int n_images, int Hs, int Ws, int* blocks, long long* span) {
    const long long total = (long long)n_images * Hs * Ws;
    long long s = (total + NLL_MAX_BLOCKS - 1) / NLL_MAX_BLOCKS;
    s = (s + 4095) / 4096 * 4096;
    *span = s;
    *blocks = (int)((total + s - 1) / s);
}

__device__ __forceinline__ int nll_target(const void* target, int dtype, long long q) {
    return dtype == IS_DTYPE_UINT8 ? (int)((const uint8_t*)target)[q] : ((const int32_t*)target)[q];
}

__global__ __launch_bounds__(NLL_THREADS) void k_nll_partials(const float* __restrict__ y, long long y_stride,
                                                              const void* __restrict__ target, int dtype, int ignore,
                                                              int n_classes, int P, long long total, long long span,
                                                              nll_partial* __restrict__ out) {
    __shared__ double sd[NLL_THREADS];
    __shared__ int sv[NLL_THREADS], sb[NLL_THREADS];
    const int tid = threadIdx.x;
    const long long beg = blockIdx.x * span, end = beg + span < total ? beg + span : total;
    double s = 0.0;
    int v = 0, b = 0;
    for (long long q = beg + tid; q < end; q += NLL_THREADS) {
        const int t = nll_target(target, dtype, q);
        const bool cls = t >= 0 && t < n_classes && t != ignore;
        const long long i = q / P, p = q - i * P;
        const float yv = y[i * y_stride + (long long)(cls ? t : 0) * P + p]; /* (the address is inside for any target) */
        if (cls) s += (double)yv, ++v;
        else if (t != ignore) ++b;
    }
    nll_tree(s, v, b, sd, sv, sb, tid);
    if (tid == 0) out[blockIdx.x] = nll_partial{s, v, b};
}

__global__ __launch_bounds__(NLL_THREADS) void k_nll_final(const nll_partial* __restrict__ in, int blocks,
                                                           float* __restrict__ loss, int32_t* __restrict__ valid,
                                                           int32_t* __restrict__ bad) {
    __shared__ double sd[NLL_THREADS];
    __shared__ int sv[NLL_THREADS], sb[NLL_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    int v = 0, b = 0;
    for (int i = tid; i < blocks; i += NLL_THREADS) s += in[i].sum, v += in[i].valid, b += in[i].bad;
    nll_tree(s, v, b, sd, sv, sb, tid);
    if (tid == 0) {
        *loss = (float)(s / (double)v); /* 0 / 0 = NaN without a valid pixel, as torch */
        *valid = v;
        *bad = b;
    }
}

__global__ __launch_bounds__(NLL_THREADS) void k_nll_grad(const void* __restrict__ target, int dtype, int ignore,
                                                          int n_classes, int P, long long total,
                                                          const int32_t* __restrict__ valid, float* __restrict__ grad,
                                                          long long grad_stride) {
    const long long q = (long long)blockIdx.x * NLL_THREADS + threadIdx.x;
    if (q >= total) return;
    const int V = *valid;
    const float unit = V > 0 ? (float)(1.0 / (double)V) : 0.0f;
    const int t = nll_target(target, dtype, q);
    const int hit = (t >= 0 && t < n_classes && t != ignore) ? t : -1;
    const long long i = q / P, p = q - i * P;
    float* g = grad + i * grad_stride + p;
    for (int c = 0; c < n_classes; ++c) g[(long long)c * P] = c == hit ? unit : 0.0f;
}

extern "C" size_t isk_semantic_nll_scratch_bytes(int n_images, int Hs, int Ws) {
    int blocks;
    long long span;
    nll_plan(n_images, Hs, Ws, &blocks, &span);
    return (size_t)blocks * sizeof(nll_partial);
}

/* The arguments are checked by is_semantic_nll (n_images * Hs * Ws fits 31 bits). */
extern "C" hipError_t isk_launch_semantic_nll(const is_semantic_nll_args* a, hipStream_t stream) {
    int blocks;
    long long span;
    nll_plan(a->n_images, a->rows8, a->cols8, &blocks, &span);
    const int P = a->rows8 * a->cols8;
    const long long total = (long long)a->n_images * P;
    nll_partial* partials = (nll_partial*)a->d_scratch;
    hipLaunchKernelGGL(k_nll_partials, dim3(blocks), dim3(NLL_THREADS), 0, stream, a->d_cnn_out, a->cnn_image_stride,
                       a->d_target, a->target_dtype, a->ignore_index, a->n_classes, P, total, span, partials);
    hipLaunchKernelGGL(k_nll_final, dim3(1), dim3(NLL_THREADS), 0, stream, (const nll_partial*)partials, blocks,
                       a->d_loss, a->d_valid_count, a->d_bad_count);
    if (a->d_grad)
        hipLaunchKernelGGL(k_nll_grad, dim3((unsigned)((total + NLL_THREADS - 1) / NLL_THREADS)), dim3(NLL_THREADS), 0,
                           stream, a->d_target, a->target_dtype, a->ignore_index, a->n_classes, P, total,
                           (const int32_t*)a->d_valid_count, a->d_grad, a->grad_image_stride);
    return hipGetLastError();
}
