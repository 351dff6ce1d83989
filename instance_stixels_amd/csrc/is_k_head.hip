/*
 * is_k_head.hip -- f13: the CNN's segmentation head of a batch in one launch (is_segmentation_head).
 *
 * What it replaces: the last three layers of the reference's models and its export wrapper,
 *   DRNDSDoubleSeg.forward (tools/CNN_training/models/DRNDownsampled.py:97-102: the 1x1 convolution `seg` from
 *   K features to n_classes + n_regression channels, -LogSoftmax over the classes, the concatenation),
 *   DRNDSOffsetDisparity.forward (:128-137: the same with a disparity channel clamped in eval mode),
 *   FlipAndPad (models/wrappers.py:35-61) and the sign of inference.py:374.
 *
 * Numerics contract:
 *   logits   z[c] = fmaf(w[c][K-1], x[K-1], ... fmaf(w[c][0], x[0], bias[c]) ...): ONE fp32 chain per (pixel, c) in
 *            increasing k, started from the bias.  No split-K, no partial sums.  v_mfma_f32_32x32x2_f32 issued in k
 *            order onto one accumulator is exactly that chain (its two k are applied low k first).  fp16 / bf16
 *            features are widened to fp32 at the load, which is exact.
 *   classes  c < n_classes: y[c] = (m + log(sum_j exp(z[j] - m))) - z[c], m = max_j z[j] over the n_classes logits,
 *            evaluated in binary64 and rounded to fp32 once.
 *   regression channels pass through; channel clamp_channel (if >= 0) is clamped to [clamp_lo, clamp_hi].
 *   d_cnn_out [n][CH][Hs][Ws] fp32 holds those values, d_segmentation [n][Ws][CH][P2S] int32 holds
 *            (int32)(8.0f * value) with the rows flipped and zero in every pad row: byte for byte k_flip_and_pad of
 *            d_cnn_out.  Every element of both is written.
 *   No atomics and no dependence on the grid: the same bytes on every run, for a frame alone and inside a batch.
 *   Non-finite logits give unspecified values; no address depends on a value.
 *
 * Tile mapping.  A workgroup of four waves owns HEAD_COLS = 32 image columns and HEAD_ROWS = 16 rows of the FLIPPED
 * row index k = Hs - 1 - row, so that the 16 ints it stores per (column, channel) are one aligned 64-byte run of
 * d_segmentation; the k tiles cover [0, P2S), and a workgroup whose rows are all pad rows only stores zeros.  A wave
 * takes four of the rows, one 32x32x2 accumulator each: channels on M (the A operand: lane l holds
 * w[c = l & 31][k0 + (l >> 5)]), the 32 pixels of a row on N (the B operand: lane l holds x[k0 + (l >> 5)][column
 * l & 31], 128 contiguous bytes per half-wave straight from global memory, no LDS).  The weights, padded to 32
 * channels with zeros, are staged in LDS HEAD_KC = 192 features at a time, transposed to [k][33] (conflict-free to fill
 * and to read); the chunks follow each other on the same accumulators, so the chain is not cut.  In the accumulator
 * a lane holds 16 channels of one pixel and lane ^ 32 the other 16: the log-softmax needs one exchange of the
 * maximum and one of the sum.  The ints go through LDS (the weights' space), 16 columns at a time, transposed to
 * [column][channel][k].
 */
#include "is_launch.h"

#define HEAD_COLS 32
#define HEAD_ROWS 16
#define HEAD_KC 192                      /* features per LDS weight chunk: 24 turns of 8 */
#define HEAD_WSTRIDE 33                  /* floats per k of the LDS weight image */
#define HEAD_TILE_WORDS (16 * (IS_HEAD_MAX_CHANNELS * HEAD_ROWS + 1)) /* the int tile of a pass at 32 channels */
#define HEAD_LDS_WORDS (HEAD_KC * HEAD_WSTRIDE > HEAD_TILE_WORDS ? HEAD_KC * HEAD_WSTRIDE : HEAD_TILE_WORDS) /* 32 832 B */
static_assert(HEAD_KC <= 256 && HEAD_KC % 24 == 0, "one thread per feature of a chunk; a full chunk is a multiple of three turns");
static_assert(IS_HEAD_MAX_CHANNELS == 32, "channels are the M side of one 32x32 tile");

typedef float head_acc __attribute__((ext_vector_type(16)));

template <int DT> struct HeadFeature;
template <> struct HeadFeature<IS_HEAD_F32> {
    typedef float type;
    static __device__ __forceinline__ float widen(float v) { return v; }
};
template <> struct HeadFeature<IS_HEAD_F16> {
    typedef _Float16 type;
    static __device__ __forceinline__ float widen(_Float16 v) { return (float)v; }
};
template <> struct HeadFeature<IS_HEAD_BF16> {
    typedef uint16_t type;
    static __device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
};

/* channel of accumulator register `reg` in the half-wave `half` (the C/D map of the 32x32 MFMA shapes) */
__device__ __forceinline__ int head_channel(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

/* One turn's features of a lane: k-step s (features 2 s + half, folded into src), row t of the wave. */
template <int DT>
__device__ __forceinline__ void head_load(float (&b)[4][4], const typename HeadFeature<DT>::type* const (&src)[4],
                                          size_t at, size_t plane) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) b[s][t] = HeadFeature<DT>::widen(src[t][at + 2 * s * plane]);
}

/* One turn's 16 MFMAs: k-step after k-step onto the same four accumulators, which is the k order of the chain. */
__device__ __forceinline__ void head_mma(head_acc (&acc)[4], const float (&b)[4][4], const float* w) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float a = w[2 * s * HEAD_WSTRIDE];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[s][t], acc[t], 0, 0, 0);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void k_head(const void* __restrict__ features_, const float* __restrict__ weight,
                                              const float* __restrict__ bias, float* __restrict__ cnn_out,
                                              int32_t* __restrict__ seg, int K, int Hs, int Ws, int n_classes,
                                              int CH, int P2S, int clamp_channel, float clamp_lo, float clamp_hi) {
    typedef typename HeadFeature<DT>::type feat_t;
    __shared__ float lds[HEAD_LDS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int w0 = blockIdx.x * HEAD_COLS, k0 = blockIdx.y * HEAD_ROWS, n = blockIdx.z;
    int32_t* seg_n = seg ? seg + (size_t)n * Ws * CH * P2S : nullptr;

    if (k0 >= Hs) { /* pad rows only */
        if (seg_n)
            for (int idx = tid; idx < HEAD_COLS * CH * HEAD_ROWS; idx += 256) {
                const int kk = idx % HEAD_ROWS, rest = idx / HEAD_ROWS, c = rest % CH, w = w0 + rest / CH;
                if (w < Ws && k0 + kk < P2S) seg_n[((size_t)w * CH + c) * P2S + k0 + kk] = 0;
            }
        return;
    }

    /* the wave's four pixels per lane: a pixel outside the image reads a pixel inside it and is never stored */
    const int w = w0 + j, wl = min(w, Ws - 1);
    const size_t plane = (size_t)Hs * Ws;
    const feat_t* src[4];
    head_acc acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row = Hs - 1 - (k0 + 4 * wave + t);
        src[t] = (const feat_t*)features_ + ((size_t)n * K + half) * plane + (size_t)max(row, 0) * Ws + wl;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = head_channel(r, half);
            const float bc = bias[min(c, CH - 1)]; /* (an unconditional load, then a select) */
            acc[t][r] = c < CH ? bc : 0.0f;
        }
    }

    /* The weights of features kc .. kc + HEAD_KC - 1 (fewer at the end of K) into LDS. */
    auto stage_weights = [&](int kc) {
        const int len = min(HEAD_KC, K - kc);
        __syncthreads();
        if (tid < len) { /* thread = feature: coalesced reads, all in flight at once, conflict-free LDS writes */
            float wv[IS_HEAD_MAX_CHANNELS];
#pragma unroll
            for (int c = 0; c < IS_HEAD_MAX_CHANNELS; ++c) wv[c] = weight[(size_t)min(c, CH - 1) * K + kc + tid];
#pragma unroll
            for (int c = 0; c < IS_HEAD_MAX_CHANNELS; ++c) lds[tid * HEAD_WSTRIDE + c] = c < CH ? wv[c] : 0.0f;
        }
        __syncthreads();
    };
    /* Four k-steps (8 features) per turn, a ring of three register sets: the loads of turn i + 2 are issued before the
     * MFMAs of turn i and stay in flight behind two turns of MFMAs, across the weight chunks too (the scheduling
     * barriers keep the compiler from sinking each load to its use).  Three turns per trip with fixed roles, so no
     * set is ever copied; a chunk is eight trips.  Past the end of K the last turn is loaded again: in bounds and
     * unused.  The one or two turns that do not fill a trip are in b0 and b1 when the loop ends. */
    const int turns = K / 8, trips = turns / 3;
    float b0[4][4], b1[4][4], b2[4][4];
    head_load<DT>(b0, src, 0, plane);
    head_load<DT>(b1, src, (size_t)min(8, K - 8) * plane, plane);
    __builtin_amdgcn_sched_barrier(0);
    for (int trip = 0; trip < trips; ++trip) {
        const int k = 24 * trip, kl = k % HEAD_KC;
        if (kl == 0) stage_weights(k);
        const float* wk = lds + (kl + half) * HEAD_WSTRIDE + j;
        head_load<DT>(b2, src, (size_t)min(k + 16, K - 8) * plane, plane);
        __builtin_amdgcn_sched_barrier(0);
        head_mma(acc, b0, wk);
        __builtin_amdgcn_sched_barrier(0);
        head_load<DT>(b0, src, (size_t)min(k + 24, K - 8) * plane, plane);
        __builtin_amdgcn_sched_barrier(0);
        head_mma(acc, b1, wk + 8 * HEAD_WSTRIDE);
        __builtin_amdgcn_sched_barrier(0);
        head_load<DT>(b1, src, (size_t)min(k + 32, K - 8) * plane, plane);
        __builtin_amdgcn_sched_barrier(0);
        head_mma(acc, b2, wk + 16 * HEAD_WSTRIDE);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (turns > 3 * trips) {
        const int k = 24 * trips, kl = k % HEAD_KC;
        if (kl == 0) stage_weights(k);
        const float* wk = lds + (kl + half) * HEAD_WSTRIDE + j;
        head_mma(acc, b0, wk);
        if (turns > 3 * trips + 1) head_mma(acc, b1, wk + 8 * HEAD_WSTRIDE);
    }

    /* epilogue 1: logits -> channel values, in place; the float output straight from the registers */
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (head_channel(r, half) < n_classes) m = fmaxf(m, acc[t][r]);
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        const double md = (double)m;
        double sum = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (8 * g < n_classes) { /* wave-uniform: no exp for a register group without a class */
#pragma unroll
                for (int r = 4 * g; r < 4 * g + 4; ++r)
                    if (head_channel(r, half) < n_classes) sum += exp((double)acc[t][r] - md);
            }
        sum += __shfl_xor(sum, 32, 64);
        const double lse = md + log(sum);
        const int k = k0 + 4 * wave + t, row = Hs - 1 - k;
        const bool inside = row >= 0 && w < Ws;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = head_channel(r, half);
            float v = acc[t][r];
            if (c < n_classes) v = (float)(lse - (double)v);
            if (c == clamp_channel) v = fminf(fmaxf(v, clamp_lo), clamp_hi);
            acc[t][r] = v;
            if (cnn_out && inside && c < CH) cnn_out[(((size_t)n * CH + c) * Hs + row) * Ws + w] = v;
        }
    }
    if (!seg_n) return;

    /* epilogue 2: (int)(8 * value), transposed through LDS to [column][channel][k], 16 columns per pass */
    int32_t* tile = (int32_t*)lds;
    const int cstride = CH * HEAD_ROWS + 1; /* odd: the 16 columns of a pass fall into different banks */
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads(); /* the weights (pass 0) or the previous pass's tile are no longer read */
        if ((j >> 4) == pass) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int kk = 4 * wave + t;
                const bool pad = k0 + kk >= Hs;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = head_channel(r, half);
                    if (c < CH) tile[(j & 15) * cstride + c * HEAD_ROWS + kk] = pad ? 0 : (int32_t)(acc[t][r] * 8.0f);
                }
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 16 * CH * HEAD_ROWS; idx += 256) {
            const int kk = idx % HEAD_ROWS, rest = idx / HEAD_ROWS, c = rest % CH, jj = rest / CH;
            const int wo = w0 + 16 * pass + jj;
            if (wo < Ws && k0 + kk < P2S)
                seg_n[((size_t)wo * CH + c) * P2S + k0 + kk] = tile[jj * cstride + c * HEAD_ROWS + kk];
        }
    }
}

/* The instantiation for a feature type (IS_HEAD_*); nullptr for any other value */
static decltype(&k_head<IS_HEAD_F32>) head_kernel(int dtype) {
    switch (dtype) {
    case IS_HEAD_F32: return k_head<IS_HEAD_F32>;
    case IS_HEAD_F16: return k_head<IS_HEAD_F16>;
    case IS_HEAD_BF16: return k_head<IS_HEAD_BF16>;
    }
    return nullptr;
}

extern "C" hipError_t isk_launch_segmentation_head(const is_segmentation_head_args* a, hipStream_t stream) {
    const int CH = a->n_classes + a->n_regression;
    const dim3 grid((a->cols8 + HEAD_COLS - 1) / HEAD_COLS,
                    (a->rows_power2_segmentation + HEAD_ROWS - 1) / HEAD_ROWS, a->n_images);
    const auto kernel = head_kernel(a->dtype);
    if (kernel == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, a->d_features, a->d_weight, a->d_bias, a->d_cnn_out,
                       a->d_segmentation, a->K, a->rows8, a->cols8, a->n_classes, CH, a->rows_power2_segmentation,
                       a->clamp_channel, a->clamp_lo, a->clamp_hi);
    return hipGetLastError();
}
