/*
 * is_k_conv3x3.hip -- f17: the backbone's tail, a dilated 3x3 convolution with folded BatchNorm and ReLU of a batch in
 * one launch (is_conv3x3_bn_relu), and the packing of its weights (is_conv3x3_pack_weights).
 * f18: the same kernel with a residual operand in its epilogue and with one tap instead of nine (is_conv_bn,
 * is_conv_pack_weights): the 3x3 convolutions and the 1x1 downsample of the residual blocks of layer5 and layer6.
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
 * f18 (BasicBlock, drn.py:54-87, built by _make_layer, drn.py:199-221, as layer5 and layer6,
 * drn.py:168-172) adds two template parameters.  The four instantiations <TAPS = 9, RESIDUAL = false> are f17's.
 *   RESIDUAL  the epilogue is v = fmaf(scale[co], a, shift[co]); v = v + (float)residual[n][co][y][x]; then max(v, 0)
 *             with relu; then the store as above.  All in fp32: two roundings, then the one of the conversion.  The
 *             residual has the features' half dtype (the widening is exact) and the OUTPUT's shape, and an element is
 *             read under exactly the predicate of its store (y < H, x < W, channel tile <= last_tile): a ragged tile
 *             and the phantom channel tile of channels_out = 32 mod 64 read nothing.
 *   TAPS = 1  the 1x1 convolution (downsample: Conv2d(1x1, bias = False) + BatchNorm2d, no ReLU).  No halo: d = 0 in
 *             every formula below, the B tile is 8 x 32 pixels, the packed layout is the same with one tap,
 *             [channel tile][chunk][k half][channel][8 k].  A wave has only 4 MFMAs per chunk, so C1_STAGE = 4
 *             16-channel chunks (fewer at the end of channels_in) are staged per barrier pair: 8 KB of weights and
 *             32 KB of pixels.  The MFMAs of an element still follow each other in increasing chunk, fixed by the
 *             shape alone.
 *
 * f19 (layer2, layer3 and layer4 of drn_d_22, drn.py:161-167 and :199-233: a stride-2 3x3 convolution,
 * and BasicBlocks whose conv1 3x3 and downsample 1x1 have stride 2) adds the template parameter STRIDE in {1, 2}.  The
 * twelve instantiations <STRIDE = 1> are f17's and f18's.
 *   STRIDE = 2  dilation 1 only.  H, W stay the INPUT's extents; the output is Ho = (H + 1) / 2 by Wo = (W + 1) / 2
 *             (torch's floor((H + 2p - d(k - 1) - 1) / 2) + 1 for k = 3, p = 1 and for k = 1, p = 0).  Output pixel
 *             (y, x) sums w[co][ci][ky][kx] * in[n][ci][2y + ky - 1][2x + kx - 1], the 1x1 form in[n][ci][2y][2x]; a
 *             tap outside the image contributes nothing.  The tile mapping, every predicate, the stores and the
 *             residual use the OUTPUT's extents; the order of the MFMAs and the epilogue are unchanged.
 *             TAPS = 9: the input tile behind 8 x 32 outputs is 17 x 65 pixels at (2 y0 - 1, 2 x0 - 1), 35.4 KB beside
 *             the 18 KB of weights.  It is stored as two column-parity planes per row, [row][33 even columns | 32 odd
 *             columns]: tap kx = 0 reads the even plane at r, kx = 1 the odd plane at r, kx = 2 the even plane at
 *             r + 1, so that the 32 lanes of every tap still read 32 CONSECUTIVE entries and hm_slot's swizzle spreads
 *             a ds_read_b128 group over all 16 slots of a bank row exactly as at stride 1.
 *             TAPS = 1: only the sampled pixels are staged, the 8 x 32 tile of in[2y][2x]; C1_STAGE as at stride 1.
 *             No address outside the features is formed for a load: a pixel outside the image loads the clamped one.
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
#include "is_half_mfma.h"

#define C3_COLS 32
#define C3_NT 2                          /* rows of a wave */
#define C3_ROWS (4 * C3_NT)              /* rows of a workgroup */
#define C3_MT 2                          /* 32-channel tiles of a workgroup */
#define C3_KC 16                         /* input channels per chunk: the k of one MFMA */
#define C3_ABLOCK(TAPS) ((TAPS) * 2 * 32) /* 16-byte units of one (channel tile, chunk) block of the packed weights */
#define C3_MAX_DILATION 8
#define C1_STAGE 4                       /* TAPS = 1: chunks staged per barrier pair */
#define C3_STAGE(TAPS) ((TAPS) == 1 ? C1_STAGE : 1)
static_assert((C3_MT * C3_ABLOCK(9) + 2 * (C3_ROWS + 2 * C3_MAX_DILATION) * (C3_COLS + 2 * C3_MAX_DILATION)) * 16 <= 65536,
              "the weights and the halo tile of the largest dilation fit the LDS a launch may ask for");
#define C3S2_ROWS (2 * C3_ROWS + 1)       /* STRIDE = 2, TAPS = 9: the input tile behind C3_ROWS x C3_COLS outputs */
#define C3S2_COLS (2 * C3_COLS + 1)
#define C3S2_EVEN (C3_COLS + 1)          /* entries of the even-column plane of a row; the odd plane has C3_COLS */
static_assert((C3_MT * C3_ABLOCK(9) + 2 * C3S2_ROWS * C3S2_COLS) * 16 <= 65536 &&
                  3 * (C3_MT * C3_ABLOCK(9) + 2 * C3S2_ROWS * C3S2_COLS) * 16 <= 160 * 1024,
              "the weights and the 17 x 65 input tile of stride 2 fit a launch's LDS, three workgroups a CU's");
static_assert(C3S2_EVEN + C3_COLS == C3S2_COLS, "the two column-parity planes of a row are the row");
static_assert(C1_STAGE * (C3_MT * C3_ABLOCK(1) + 2 * C3_ROWS * C3_COLS) * 16 <= 65536, "and so does a stage of the 1x1 form");

/* packed[((tile * chunks + chunk) * taps + tap) * 512 + h * 256 + r * 8 + j] = round(w[32 tile + r][16 chunk + 8 h + j][tap]) */
template <int DT>
__global__ __launch_bounds__(256) void k_conv3x3_pack(const float* __restrict__ weight, uint16_t* __restrict__ packed,
                                                      int Cin, int taps, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = e & 7, r = (e >> 3) & 31, h = (e >> 8) & 1, tap = (e >> 9) % taps, blk = (e >> 9) / taps;
    const int chunks = Cin / C3_KC, chunk = blk % chunks, tile = blk / chunks;
    const int co = 32 * tile + r, ci = C3_KC * chunk + 8 * h + j;
    packed[e] = hm_round<DT>(weight[((size_t)co * Cin + ci) * taps + tap]);
}

/* H, W: the INPUT's extents (STRIDE = 1: the output's as well). */
template <int DT, bool F32OUT, int TAPS, bool RESIDUAL, int STRIDE>
__global__ __launch_bounds__(256) void k_conv3x3(const uint16_t* __restrict__ features, const uint4* __restrict__ packed,
                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                 const uint16_t* __restrict__ residual, void* __restrict__ out_, int Cin,
                                                 int Cout, int H, int W, int d_, int relu, int tiles_x, int tiles,
                                                 int groups) {
    static_assert(TAPS == 9 || TAPS == 1, "a 3x3 or a 1x1 convolution");
    static_assert(STRIDE == 1 || STRIDE == 2, "stride 1, or stride 2 at dilation 1");
    constexpr int ABLOCK = C3_ABLOCK(TAPS), STAGE = C3_STAGE(TAPS);
    constexpr bool PARITY = STRIDE == 2 && TAPS == 9; /* the B tile is the 17 x 65 input tile in column-parity planes */
    const int d = TAPS == 1 ? 0 : STRIDE == 2 ? 1 : d_;
    const int Ho = STRIDE == 2 ? (H + 1) / 2 : H, Wo = STRIDE == 2 ? (W + 1) / 2 : W; /* the output's extents */
    extern __shared__ uint4 c3_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;
    /* workgroup b of the grid runs on XCD b & 7: the channel groups of a pixel tile follow each other there */
    const int seq = blockIdx.x >> 3, group = seq % groups, tile = (seq / groups) * 8 + (blockIdx.x & 7);
    if (tile >= tiles) return; /* (the whole workgroup, before any barrier) */
    const int n = blockIdx.y, y0 = (tile / tiles_x) * C3_ROWS, x0 = (tile % tiles_x) * C3_COLS;
    const int HW = PARITY ? C3S2_COLS : C3_COLS + 2 * d, pixels = (PARITY ? C3S2_ROWS : C3_ROWS + 2 * d) * HW;
    const int chunks = Cin / C3_KC;
    uint4* const ldsA = c3_lds;                          /* [C3_MT][chunk of the stage][tap][k half][channel] */
    uint4* const ldsB = c3_lds + C3_MT * STAGE * ABLOCK; /* [chunk of the stage] hm_slot(pixel, k half) */
    const size_t plane = (size_t)H * W;
    const uint16_t* const xn = features + (size_t)n * Cin * plane;
    const int last_tile = Cout / 32 - 1;

    hm_acc16 acc[C3_MT][C3_NT];
#pragma unroll
    for (int m = 0; m < C3_MT; ++m)
#pragma unroll
        for (int t = 0; t < C3_NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][t][i] = 0.0f;

    for (int chunk = 0; chunk < chunks; chunk += STAGE) {
        const int nc = STAGE == 1 ? 1 : min(STAGE, chunks - chunk); /* chunks of this stage */
        __syncthreads(); /* the previous stage's operands are no longer read */
        /* A: a channel tile past the last one (channels_out = 32 mod 64) copies the last one and is never stored */
#pragma unroll
        for (int m = 0; m < C3_MT; ++m) {
            const uint4* src = packed + ((size_t)min(C3_MT * group + m, last_tile) * chunks + chunk) * ABLOCK;
            for (int i = tid; i < nc * ABLOCK; i += 256) ldsA[m * STAGE * ABLOCK + i] = src[i];
        }
        /* B: an item is 8 channels of one halo pixel; consecutive threads take consecutive pixels of a plane.  A pixel
         * outside the image loads the nearest pixel inside it and stores zeros.  STRIDE = 2: tile pixel (py, px) is
         * input pixel (2 y0 - 1 + py, 2 x0 - 1 + px), stored at its column parity's plane; the 1x1 form takes the
         * sampled pixels (2 (y0 + py), 2 (x0 + px)) alone. */
        for (int it_ = tid; it_ < nc * 2 * pixels; it_ += 256) {
            const int cc = STAGE == 1 ? 0 : it_ / (2 * pixels), it = it_ - cc * 2 * pixels;
            const int h = it >= pixels, p = it - h * pixels, py = p / HW, px = p - py * HW;
            const int gy = STRIDE == 1 ? y0 - d + py : TAPS == 9 ? 2 * y0 - 1 + py : 2 * (y0 + py);
            const int gx = STRIDE == 1 ? x0 - d + px : TAPS == 9 ? 2 * x0 - 1 + px : 2 * (x0 + px);
            const int lp = PARITY ? py * C3S2_COLS + (px & 1) * C3S2_EVEN + (px >> 1) : p;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const uint16_t* src = xn + (size_t)(C3_KC * (chunk + cc) + 8 * h) * plane +
                                  (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = src[j * plane];
            uint4 q;
            q.x = v[0] | (v[1] << 16), q.y = v[2] | (v[3] << 16), q.z = v[4] | (v[5] << 16), q.w = v[6] | (v[7] << 16);
            ldsB[cc * 2 * pixels + hm_slot(lp, h)] = inside ? q : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        for (int cc = 0; cc < nc; ++cc) {
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int ky = tap / 3, kx = tap % 3;
                uint4 a[C3_MT], b[C3_NT];
#pragma unroll
                for (int m = 0; m < C3_MT; ++m) a[m] = ldsA[(m * STAGE + cc) * ABLOCK + (2 * tap + half) * 32 + r];
#pragma unroll
                for (int t = 0; t < C3_NT; ++t) {
                    /* PARITY: input row 2 (row of the tile) + ky; column 2 r + kx is entry r + kx / 2 of plane kx & 1 */
                    const int bp = PARITY ? (2 * (C3_NT * wave + t) + ky) * C3S2_COLS + (kx & 1) * C3S2_EVEN + (kx >> 1) + r
                                          : (C3_NT * wave + t + ky * d) * HW + r + kx * d;
                    b[t] = ldsB[cc * 2 * pixels + hm_slot(bp, half)];
                }
#pragma unroll
                for (int m = 0; m < C3_MT; ++m)
#pragma unroll
                    for (int t = 0; t < C3_NT; ++t) acc[m][t] = hm_mfma<DT>(a[m], b[t], acc[m][t]);
            }
        }
    }

    /* epilogue: register i of a lane is channel hm_cd_row(i, half) of its tile at the lane's pixel: 32 lanes store 32
     * consecutive elements of a plane */
    const int x = x0 + r;
#pragma unroll
    for (int m = 0; m < C3_MT; ++m) {
        const int tile_m = C3_MT * group + m;
        if (tile_m > last_tile) break;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = 32 * tile_m + hm_cd_row(i, half);
            const float sc = scale[co], sh = shift[co];
#pragma unroll
            for (int t = 0; t < C3_NT; ++t) {
                const int y = y0 + C3_NT * wave + t;
                float v = fmaf(sc, acc[m][t][i], sh);
                if (RESIDUAL) { /* (read under the predicate of the store below, at the store's index) */
                    if (y < Ho && x < Wo) v = v + hm_widen<DT>(residual[(((size_t)n * Cout + co) * Ho + y) * Wo + x]);
                }
                if (relu) v = fmaxf(v, 0.0f);
                if (y < Ho && x < Wo) {
                    const size_t at = (((size_t)n * Cout + co) * Ho + y) * Wo + x;
                    if (F32OUT) ((float*)out_)[at] = v;
                    else ((uint16_t*)out_)[at] = hm_round<DT>(v);
                }
            }
        }
    }
}

/* The arguments are checked by is_conv_pack_weights. */
extern "C" hipError_t isk_launch_conv_pack(const float* d_weight, int channels_out, int channels_in, int kernel, int dtype,
                                           void* d_packed, hipStream_t stream) {
    const int taps = kernel * kernel, total = channels_out * channels_in * taps; /* at most 2048 * 2048 * 9 */
    const dim3 grid((total + 255) / 256);
    const bool half = hm_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_conv3x3_pack<dt()>, grid, dim3(256), 0, stream, d_weight, (uint16_t*)d_packed, channels_in, taps, total);
    });
    if (!half) return hipErrorInvalidValue;
    return hipGetLastError();
}

template <int DT, bool F32OUT, int TAPS, bool RESIDUAL, int STRIDE>
static void c3_launch(const is_conv_bn_stride_args* a, hipStream_t stream) {
    const int d = TAPS == 1 ? 0 : a->dilation;
    const int rows_out = (a->rows_in + STRIDE - 1) / STRIDE, cols_out = (a->cols_in + STRIDE - 1) / STRIDE;
    const int tiles_x = (cols_out + C3_COLS - 1) / C3_COLS, tiles = tiles_x * ((rows_out + C3_ROWS - 1) / C3_ROWS);
    const int groups = (a->channels_out / 32 + C3_MT - 1) / C3_MT;
    const dim3 grid((unsigned)groups * (unsigned)((tiles + 7) / 8 * 8), a->n_images); /* at most 32 * 2^22 */
    const size_t b_pixels = STRIDE == 2 && TAPS == 9 ? C3S2_ROWS * C3S2_COLS : (C3_ROWS + 2 * d) * (C3_COLS + 2 * d);
    const size_t lds = (size_t)C3_STAGE(TAPS) * (C3_MT * C3_ABLOCK(TAPS) + 2 * b_pixels) * 16;
    hipLaunchKernelGGL((k_conv3x3<DT, F32OUT, TAPS, RESIDUAL, STRIDE>), grid, dim3(256), lds, stream,
                       (const uint16_t*)a->d_features, (const uint4*)a->d_packed, a->d_scale, a->d_shift,
                       (const uint16_t*)a->d_residual, a->d_out, a->channels_in, a->channels_out, a->rows_in, a->cols_in, d,
                       a->relu, tiles_x, tiles, groups);
}

/* The arguments are checked by is_core.hip's conv_bn_run, for is_conv_bn_stride, is_conv_bn and is_conv3x3_bn_relu alike. */
extern "C" hipError_t isk_launch_conv_bn(const is_conv_bn_stride_args* a, hipStream_t stream) {
    const bool f32out = a->out_dtype == IS_HEAD_F32;
    if ((a->kernel != 3 && a->kernel != 1) || (a->stride != 1 && a->stride != 2)) return hipErrorInvalidValue;
    const bool half = hm_dispatch(a->dtype, [&](auto dt) {
        hm_either<true, false>(f32out, [&](auto f32) {
            hm_either<9, 1>(a->kernel == 3, [&](auto taps) {
                hm_either<2, 1>(a->stride == 2, [&](auto stride) {
                    hm_either<true, false>(a->d_residual != nullptr, [&](auto residual) {
                        c3_launch<dt(), f32(), taps(), residual(), stride()>(a, stream);
                    });
                });
            });
        });
    });
    if (!half) return hipErrorInvalidValue;
    return hipGetLastError();
}
