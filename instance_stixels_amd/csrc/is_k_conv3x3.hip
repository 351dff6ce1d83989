/*
 * is_k_conv3x3.hip -- f17: the backbone's tail, a dilated 3x3 convolution with folded BatchNorm and ReLU of a batch in
 * one launch (is_conv3x3_bn_relu), and the packing of its weights (is_conv3x3_pack_weights).
 *
 * What it replaces: layer7 and layer8 of the reference's DRN (tools/CNN_training/models/drn.py:181-185, built by
 *   _make_conv_layers, :223-233: Conv2d(C, C, 3, padding = dilation, dilation, bias = False) + BatchNorm2d + ReLU),
 *   which the reference runs in half precision (inference.py:278).  layer7 -> layer8 -> is_segmentation_head is three
 *   launches of this library with nothing in between.
 *
 * Numerics contract:
 *   operands  the half values: the features as given, the weights as is_conv3x3_pack_weights rounded them (round to
 *             nearest even).  A product of two of them is exact in fp32.
 *   sum       a[n][co][y][x] = sum over the 9 taps and all channels_in of
 *             w[co][ci][ky][kx] * x[n][ci][y + (ky - 1) d][x + (kx - 1) d]; a tap outside the image contributes
 *             nothing.  Accumulated in fp32 by v_mfma_f32_32x32x16_{f16,bf16} on ONE accumulator per output element:
 *             no split over workgroups, no atomics, no partial sums combined afterwards.
 *   order     the MFMA instructions of an element follow each other in increasing 16-channel chunk and, inside a
 *             chunk, in increasing tap 3 ky + kx: fixed by the shape alone.  The summation of the 16 products INSIDE
 *             one instruction is the hardware's and is not specified, so this entry point is pinned by a derived bound
 *             and by inputs whose arithmetic is exact in every order -- not by a C loop, as f13's stronger contract is.
 *   epilogue  v = fmaf(scale[co], a, shift[co]) in fp32, then max(v, 0) with relu; stored as fp32, or converted to the
 *             half dtype round to nearest even.
 *   The same bytes on every run; a frame's result does not depend on its position in the batch or on n_images.
 *   Non-finite values give unspecified values; no address depends on a value.
 *
 * Tile mapping.  A workgroup of four waves owns C3_MT = 2 tiles of 32 output channels and C3_ROWS = 8 rows of
 * C3_COLS = 32 pixels of one frame; a wave takes two of the rows and holds 2 x 2 accumulators of 32x32x16: output
 * channels on M, the 32 pixels of a row on N, so that an accumulator register is 32 consecutive pixels of one NCHW
 * plane.  The input channels go by in chunks of 16 (one MFMA's k).  Per chunk the workgroup stages
 *   A  the weights of its 64 channels, 9 taps: a plain 16-byte copy of the packed layout
 *      [channel tile][chunk][tap][k half][channel][8 k], which is the A fragment lane by lane (ds_read_b128 of
 *      consecutive lanes: consecutive 16 bytes);
 *   B  the halo tile of (8 + 2d) x (32 + 2d) pixels channel-innermost, [pixel][2 k halves of 8 channels], zero-filled
 *      outside the image: every tap of every pixel, border or interior, dilation above the image size or not, is the
 *      same ds_read_b128 at a 16-byte aligned address (no transposed read at a shifted address).  The two 16-byte
 *      slots of a pixel are swapped where bit 3 of the pixel index is set: the 16 lanes of a ds_read_b128 group read
 *      16 consecutive pixels, whose slots then cover all 16 slots of a bank row.
 * Then 9 taps x 4 MFMAs per wave.  Consecutive workgroups of one XCD (every eighth of the grid) take the channel groups
 * of ONE pixel tile, so the tile's features come from memory once and from L2 for the other channel groups.
 */
#include "is_launch.h"

#define C3_COLS 32
#define C3_NT 2                          /* rows of a wave */
#define C3_ROWS (4 * C3_NT)              /* rows of a workgroup */
#define C3_MT 2                          /* 32-channel tiles of a workgroup */
#define C3_KC 16                         /* input channels per chunk: the k of one MFMA */
#define C3_ABLOCK (9 * 2 * 32)           /* 16-byte units of one (channel tile, chunk) block of the packed weights */
#define C3_MAX_DILATION 8
static_assert((C3_MT * C3_ABLOCK + 2 * (C3_ROWS + 2 * C3_MAX_DILATION) * (C3_COLS + 2 * C3_MAX_DILATION)) * 16 <= 65536,
              "the weights and the halo tile of the largest dilation fit the LDS a launch may ask for");

typedef float c3_acc __attribute__((ext_vector_type(16)));
typedef _Float16 c3_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 c3_bf16x8 __attribute__((ext_vector_type(8)));

/* fp32 -> half, round to nearest even, as 16 bits */
template <int DT> __device__ __forceinline__ uint16_t c3_round(float v);
template <> __device__ __forceinline__ uint16_t c3_round<IS_HEAD_F16>(float v) {
    return __builtin_bit_cast(uint16_t, (_Float16)v);
}
template <> __device__ __forceinline__ uint16_t c3_round<IS_HEAD_BF16>(float v) {
    const uint32_t u = __float_as_uint(v);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <int DT> __device__ __forceinline__ c3_acc c3_mfma(uint4 a, uint4 b, c3_acc c);
template <> __device__ __forceinline__ c3_acc c3_mfma<IS_HEAD_F16>(uint4 a, uint4 b, c3_acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(c3_f16x8, a), __builtin_bit_cast(c3_f16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ c3_acc c3_mfma<IS_HEAD_BF16>(uint4 a, uint4 b, c3_acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(c3_bf16x8, a), __builtin_bit_cast(c3_bf16x8, b), c, 0, 0, 0);
}

/* the 16-byte slot of k half `h` of halo pixel `p` */
__device__ __forceinline__ int c3_slot(int p, int h) { return 2 * p + (h ^ ((p >> 3) & 1)); }

/* packed[((tile * chunks + chunk) * 9 + tap) * 512 + h * 256 + r * 8 + j] = round(w[32 tile + r][16 chunk + 8 h + j][tap]) */
template <int DT>
__global__ __launch_bounds__(256) void k_conv3x3_pack(const float* __restrict__ weight, uint16_t* __restrict__ packed,
                                                      int Cin, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = e & 7, r = (e >> 3) & 31, h = (e >> 8) & 1, tap = (e >> 9) % 9, blk = (e >> 9) / 9;
    const int chunks = Cin / C3_KC, chunk = blk % chunks, tile = blk / chunks;
    const int co = 32 * tile + r, ci = C3_KC * chunk + 8 * h + j;
    packed[e] = c3_round<DT>(weight[((size_t)co * Cin + ci) * 9 + tap]);
}

template <int DT, bool F32OUT>
__global__ __launch_bounds__(256) void k_conv3x3(const uint16_t* __restrict__ features, const uint4* __restrict__ packed,
                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                 void* __restrict__ out_, int Cin, int Cout, int H, int W, int d,
                                                 int relu, int tiles_x, int tiles, int groups) {
    extern __shared__ uint4 c3_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;
    /* workgroup b of the grid runs on XCD b & 7: the channel groups of a pixel tile follow each other there */
    const int seq = blockIdx.x >> 3, group = seq % groups, tile = (seq / groups) * 8 + (blockIdx.x & 7);
    if (tile >= tiles) return; /* (the whole workgroup, before any barrier) */
    const int n = blockIdx.y, y0 = (tile / tiles_x) * C3_ROWS, x0 = (tile % tiles_x) * C3_COLS;
    const int HW = C3_COLS + 2 * d, pixels = (C3_ROWS + 2 * d) * HW, chunks = Cin / C3_KC;
    uint4* const ldsA = c3_lds;                    /* [C3_MT][tap][k half][channel] */
    uint4* const ldsB = c3_lds + C3_MT * C3_ABLOCK; /* c3_slot(pixel, k half) */
    const size_t plane = (size_t)H * W;
    const uint16_t* const xn = features + (size_t)n * Cin * plane;
    const int last_tile = Cout / 32 - 1;

    c3_acc acc[C3_MT][C3_NT];
#pragma unroll
    for (int m = 0; m < C3_MT; ++m)
#pragma unroll
        for (int t = 0; t < C3_NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][t][i] = 0.0f;

    for (int chunk = 0; chunk < chunks; ++chunk) {
        __syncthreads(); /* the previous chunk's operands are no longer read */
        /* A: a channel tile past the last one (channels_out = 32 mod 64) copies the last one and is never stored */
#pragma unroll
        for (int m = 0; m < C3_MT; ++m) {
            const uint4* src = packed + ((size_t)min(C3_MT * group + m, last_tile) * chunks + chunk) * C3_ABLOCK;
            for (int i = tid; i < C3_ABLOCK; i += 256) ldsA[m * C3_ABLOCK + i] = src[i];
        }
        /* B: an item is 8 channels of one halo pixel; consecutive threads take consecutive pixels of a plane.  A pixel
         * outside the image loads the nearest pixel inside it and stores zeros. */
        for (int it = tid; it < 2 * pixels; it += 256) {
            const int h = it >= pixels, p = it - h * pixels, py = p / HW, px = p - py * HW;
            const int gy = y0 - d + py, gx = x0 - d + px;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const uint16_t* src = xn + (size_t)(C3_KC * chunk + 8 * h) * plane +
                                  (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = src[j * plane];
            uint4 q;
            q.x = v[0] | (v[1] << 16), q.y = v[2] | (v[3] << 16), q.z = v[4] | (v[5] << 16), q.w = v[6] | (v[7] << 16);
            ldsB[c3_slot(p, h)] = inside ? q : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            uint4 a[C3_MT], b[C3_NT];
#pragma unroll
            for (int m = 0; m < C3_MT; ++m) a[m] = ldsA[m * C3_ABLOCK + (2 * tap + half) * 32 + r];
#pragma unroll
            for (int t = 0; t < C3_NT; ++t)
                b[t] = ldsB[c3_slot((C3_NT * wave + t + ky * d) * HW + r + kx * d, half)];
#pragma unroll
            for (int m = 0; m < C3_MT; ++m)
#pragma unroll
                for (int t = 0; t < C3_NT; ++t) acc[m][t] = c3_mfma<DT>(a[m], b[t], acc[m][t]);
        }
    }

    /* epilogue: register i of a lane is channel (i & 3) + 8 (i >> 2) + 4 half of its tile (the C/D map of the 32x32
     * shapes) at the lane's pixel: 32 lanes store 32 consecutive elements of a plane */
    const int x = x0 + r;
#pragma unroll
    for (int m = 0; m < C3_MT; ++m) {
        const int tile_m = C3_MT * group + m;
        if (tile_m > last_tile) break;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = 32 * tile_m + (i & 3) + 8 * (i >> 2) + 4 * half;
            const float sc = scale[co], sh = shift[co];
#pragma unroll
            for (int t = 0; t < C3_NT; ++t) {
                const int y = y0 + C3_NT * wave + t;
                float v = fmaf(sc, acc[m][t][i], sh);
                if (relu) v = fmaxf(v, 0.0f);
                if (y < H && x < W) {
                    const size_t at = (((size_t)n * Cout + co) * H + y) * W + x;
                    if (F32OUT) ((float*)out_)[at] = v;
                    else ((uint16_t*)out_)[at] = c3_round<DT>(v);
                }
            }
        }
    }
}

/* The arguments are checked by is_conv3x3_pack_weights. */
extern "C" hipError_t isk_launch_conv3x3_pack(const float* d_weight, int channels_out, int channels_in, int dtype,
                                              void* d_packed, hipStream_t stream) {
    const int total = channels_out * channels_in * 9; /* at most 2048 * 2048 * 9 */
    const dim3 grid((total + 255) / 256);
    if (dtype == IS_HEAD_F16)
        hipLaunchKernelGGL(k_conv3x3_pack<IS_HEAD_F16>, grid, dim3(256), 0, stream, d_weight, (uint16_t*)d_packed, channels_in, total);
    else if (dtype == IS_HEAD_BF16)
        hipLaunchKernelGGL(k_conv3x3_pack<IS_HEAD_BF16>, grid, dim3(256), 0, stream, d_weight, (uint16_t*)d_packed, channels_in, total);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

/* The arguments are checked by is_conv3x3_bn_relu. */
extern "C" hipError_t isk_launch_conv3x3(const is_conv3x3_args* a, hipStream_t stream) {
    const int d = a->dilation;
    const int tiles_x = (a->cols8 + C3_COLS - 1) / C3_COLS, tiles = tiles_x * ((a->rows8 + C3_ROWS - 1) / C3_ROWS);
    const int groups = (a->channels_out / 32 + C3_MT - 1) / C3_MT;
    const dim3 grid((unsigned)groups * (unsigned)((tiles + 7) / 8 * 8), a->n_images); /* at most 32 * 2^22 */
    const size_t lds = (size_t)(C3_MT * C3_ABLOCK + 2 * (C3_ROWS + 2 * d) * (C3_COLS + 2 * d)) * 16;
    const bool f32out = a->out_dtype == IS_HEAD_F32;
#define C3_LAUNCH(DT, F32)                                                                                           \
    hipLaunchKernelGGL((k_conv3x3<DT, F32>), grid, dim3(256), lds, stream, (const uint16_t*)a->d_features,            \
                       (const uint4*)a->d_packed, a->d_scale, a->d_shift, a->d_out, a->channels_in, a->channels_out, \
                       a->rows8, a->cols8, d, a->relu, tiles_x, tiles, groups)
    if (a->dtype == IS_HEAD_F16) {
        if (f32out) C3_LAUNCH(IS_HEAD_F16, true); else C3_LAUNCH(IS_HEAD_F16, false);
    } else if (a->dtype == IS_HEAD_BF16) {
        if (f32out) C3_LAUNCH(IS_HEAD_BF16, true); else C3_LAUNCH(IS_HEAD_BF16, false);
    } else {
        return hipErrorInvalidValue;
    }
#undef C3_LAUNCH
    return hipGetLastError();
}
