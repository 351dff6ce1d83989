/*
 * is_k_stem.hip -- f20: the backbone's stem of a batch in one launch (is_stem), from the camera's bytes to layer1's
 * output, and the packing of its two weights (is_stem_pack_weights).
 *
 * What it replaces: layer0 and layer1 of the reference's drn_d_22 (tools/CNN_training/models/drn.py:154-159: Conv2d(3,
 *   16, 7, stride 1, padding 3, bias = False) + BatchNorm2d + ReLU; drn.py:161-162, _make_conv_layers with layers[0]
 *   == 1: Conv2d(16, 16, 3, padding 1, bias = False) + BatchNorm2d + ReLU) and, in front of them, ToTensor + Normalize
 *   + the cast to half of the image (inference.py:109-110, :278).  is_stem -> is_conv_bn_stride x 23 ->
 *   is_segmentation_head is 25 launches of this library with nothing in between: image bytes in, the DP's input out.
 *
 * Numerics contract:
 *   x[n][c][y][x]  = lut[c][ image[n][y][x][c] ]                       c in 0..2
 *   mid            = half( relu( bn0( conv7x7(x), pad 3 ) ) )          3 -> 16 channels
 *   out            = half( relu( bn1( conv3x3(mid), pad 1 ) ) )        16 -> 16 channels
 *   input     d_image is uint8 [n_images][rows][cols][3], interleaved and contiguous; d_lut is [3][256] of the half
 *             dtype.  The operand of layer0 at channel c is lut[c][byte]: that is the whole definition of the
 *             normalisation, and the kernel gives the table's bits (it keeps the table in LDS).  Byte position c pairs
 *             with input channel c of layer0's weight.
 *   padding of layer0   a tap outside the image contributes nothing: zero padding of the NORMALISED value, not
 *             lut[c][0]; it cannot be folded into weights or shift.
 *   mid       a0 = sum over 3 x 7 x 7 of w0[co][ci][ky][kx] * x[n][ci][y + ky - 3][x + kx - 3] in fp32 by
 *             v_mfma_f32_16x16x32_{f16,bf16} on ONE accumulator per element: seven instructions in increasing ky, fixed
 *             by the shape alone; an instruction holds k = (kx in 0..7, ci in 0..3), and the slots kx = 7 and ci = 3
 *             are exact zeros on both operands.  The order inside one instruction is the hardware's, as in f17.  Then
 *             v = fmaf(scale0[co], a0, shift0[co]), max(v, 0), rounded to the half dtype to nearest even.  layer1's
 *             operands are exactly these half values.
 *   padding of layer1   a mid pixel OUTSIDE THE IMAGE IS ZERO: not relu(shift0) and not a convolution evaluated past
 *             the edge.
 *   out       a1 = sum over 16 x 3 x 3 of w1[co][ci][ky][kx] * mid[n][ci][y + ky - 1][x + kx - 1], five instructions in
 *             increasing k = 16 (3 ky + kx) + ci, the slots k >= 144 exact zeros on both operands; then
 *             fmaf(scale1[co], a1, shift1[co]), max(., 0), rounded to nearest even.  d_out is [n][16][rows][cols],
 *             what is_conv_bn_stride reads for layer2; every element is written.
 *   d_mid     NULL, or [n][16][rows][cols] of the half dtype: every element of mid is also stored, by the workgroup
 *             that owns the pixel.  d_out has the same bytes whether or not d_mid is given; with d_mid == NULL mid
 *             never reaches global memory.  A mid halo pixel computed by two workgroups has the same bits in both:
 *             the same seven instructions in the same order on the same operands.
 *   The same bytes on every run; a frame's result does not depend on its position in the batch or on n_images; no
 *   atomics.  No address outside the image's n * rows * cols * 3 bytes is loaded from: a pixel outside the image loads
 *   the clamped one and stores zeros.  Non-finite table entries give unspecified values and never a wild access: no
 *   address depends on a value other than the table index, which is a byte.
 *
 * Tile mapping.  A workgroup of four waves owns ST_ROWS = 16 rows of ST_COLS = 64 output pixels of one frame.
 *   1  the table to LDS (1.5 KB);
 *   2  the byte tile with a halo of 4, (16 + 8) x (64 + 8) pixels, looked up: [pixel][ci 0..2, 0] halves, 8 bytes a
 *      pixel, zeros outside the image (13.9 KB);
 *   3  mid on the tile plus a halo of 1, 18 x 66 = 1188 pixels taken as 75 groups of 16 CONSECUTIVE pixels of that
 *      list (no group is wasted on a row's end), channels on M and pixels on N: lane (p = lane & 15, g = lane >> 4)
 *      reads for step ky the 16 bytes of the two pixels (row + ky, col + 2g), (row + ky, col + 2g + 1), its eight k
 *      values kx = 2g + (j >> 2), ci = j & 3; its four results are channels 4g .. 4g + 3 of pixel p, one 8-byte LDS
 *      write into [pixel][16 channels] (38 KB), zeros for a pixel outside the image;
 *   4  out from LDS, 64 groups of 16 pixels of a row, PIXELS on M and channels on N: the A fragment of step s is the
 *      16 bytes of channels 8 (g & 1) .. + 7 of pixel p at tap 2s + (g >> 1), and a lane's four results are four
 *      consecutive pixels of ONE channel plane, one 8-byte store.
 *   The weights never touch LDS: the packed blob is the 7 + 5 fragments lane by lane, 48 registers for the launch.
 */
#include "is_half_mfma.h"

#define ST_ROWS 16
#define ST_COLS 64
#define ST_XROWS (ST_ROWS + 8)              /* the looked-up tile: a halo of 4 (3 of layer0 behind 1 of layer1) */
#define ST_XCOLS (ST_COLS + 8)
#define ST_XPIX (ST_XROWS * ST_XCOLS + 8)   /* + the pixel that the zero slot kx = 7 of the last pixel reads */
#define ST_MROWS (ST_ROWS + 2)              /* mid: a halo of 1 */
#define ST_MCOLS (ST_COLS + 2)
#define ST_MPIX (ST_MROWS * ST_MCOLS)
#define ST_MGROUPS ((ST_MPIX + 15) / 16)    /* groups of 16 consecutive mid pixels */
#define ST_OGROUPS (ST_ROWS * ST_COLS / 16)
#define ST_K0 7                             /* MFMA steps of layer0: one per ky */
#define ST_K1 5                             /* of layer1: k = 16 tap + ci, 144 padded to 160 */
#define ST_LDS_BYTES (3 * 256 * 2 + ST_XPIX * 8 + ST_MPIX * 32)
static_assert(ST_LDS_BYTES <= 65536 && 3 * ST_LDS_BYTES <= 160 * 1024,
              "the table, the looked-up tile and mid fit the LDS a launch may ask for, three workgroups a CU's");
static_assert(ST_COLS % 16 == 0 && ST_OGROUPS % 4 == 0, "an output group is 16 pixels of one row; four waves share them");
static_assert((ST_XROWS - 1) * ST_XCOLS + (ST_MCOLS - 1) + 2 * 3 + 1 < ST_XPIX, "the last read of layer0 is inside the tile");

/* The blob, in 16-bit elements e = (step * 64 + lane) * 8 + j, the fragment of `lane` in `step`:
 *   step < 7   layer0, ky = step: round(w0[lane & 15][j & 3][ky][2 (lane >> 4) + (j >> 2)]), 0 where ci = 3 or kx = 7
 *   step >= 7  layer1, s = step - 7, k = 32 s + 8 (lane >> 4) + j = 16 tap + ci: round(w1[lane & 15][ci][tap / 3][tap % 3]),
 *              0 where tap = 9 */
template <int DT>
__global__ __launch_bounds__(256) void k_stem_pack(const float* __restrict__ w0, const float* __restrict__ w1,
                                                   uint16_t* __restrict__ packed) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (ST_K0 + ST_K1) * 64 * 8) return;
    const int j = e & 7, lane = (e >> 3) & 63, step = e >> 9, co = lane & 15, g = lane >> 4;
    float v = 0.0f;
    if (step < ST_K0) {
        const int ci = j & 3, kx = 2 * g + (j >> 2);
        if (ci < 3 && kx < 7) v = w0[((co * 3 + ci) * 7 + step) * 7 + kx];
    } else {
        const int k = 32 * (step - ST_K0) + 8 * g + j, tap = k >> 4, ci = k & 15;
        if (tap < 9) v = w1[(co * 16 + ci) * 9 + tap];
    }
    packed[e] = hm_round<DT>(v);
}

template <int DT>
__global__ __launch_bounds__(256) void k_stem(const uint8_t* __restrict__ image, const uint16_t* __restrict__ lut,
                                              const uint4* __restrict__ packed, const float* __restrict__ scale0,
                                              const float* __restrict__ shift0, const float* __restrict__ scale1,
                                              const float* __restrict__ shift1, uint16_t* __restrict__ mid_out,
                                              uint16_t* __restrict__ out, int H, int W, int tiles_x) {
    __shared__ uint16_t s_lut[3 * 256];
    __shared__ uint2 s_x[ST_XPIX];         /* [pixel of the looked-up tile] (ci 0, ci 1), (ci 2, 0) */
    __shared__ uint4 s_mid[2 * ST_MPIX];   /* hm_slot(pixel of the mid tile, channel half) */
    static_assert(sizeof(s_lut) + sizeof(s_x) + sizeof(s_mid) == ST_LDS_BYTES, "the LDS account of the header");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, g = lane >> 4;
    const int n = blockIdx.y, y0 = (blockIdx.x / tiles_x) * ST_ROWS, x0 = (blockIdx.x % tiles_x) * ST_COLS;
    const size_t plane = (size_t)H * W;
    const uint8_t* const img = image + (size_t)n * plane * 3;

    /* the fragments of the weights, and the folds of the lane's channels: 4g .. 4g + 3 in layer0, p in layer1 */
    uint4 w0[ST_K0], w1[ST_K1];
#pragma unroll
    for (int s = 0; s < ST_K0; ++s) w0[s] = packed[s * 64 + lane];
#pragma unroll
    for (int s = 0; s < ST_K1; ++s) w1[s] = packed[(ST_K0 + s) * 64 + lane];
    float sc0[4], sh0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sc0[i] = scale0[4 * g + i], sh0[i] = shift0[4 * g + i];
    const float sc1 = scale1[p], sh1 = shift1[p];

    /* 1: the table */
    for (int i = tid; i < 3 * 256; i += 256) s_lut[i] = lut[i];
    if (tid < ST_XPIX - ST_XROWS * ST_XCOLS) s_x[ST_XROWS * ST_XCOLS + tid] = make_uint2(0, 0);
    __syncthreads();

    /* 2: the looked-up tile.  Consecutive threads take consecutive pixels of a row: consecutive 3 bytes.  A pixel
     * outside the image loads the nearest pixel inside it and stores zeros. */
    for (int it = tid; it < ST_XROWS * ST_XCOLS; it += 256) {
        const int py = it / ST_XCOLS, px = it - py * ST_XCOLS, gy = y0 - 4 + py, gx = x0 - 4 + px;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const uint8_t* src = img + ((size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * 3;
        const uint32_t b0 = src[0], b1 = src[1], b2 = src[2];
        const uint2 q = make_uint2((uint32_t)s_lut[b0] | ((uint32_t)s_lut[256 + b1] << 16), (uint32_t)s_lut[512 + b2]);
        s_x[it] = inside ? q : make_uint2(0, 0);
    }
    __syncthreads();

    /* 3: mid on the tile plus a halo of 1 */
    for (int grp = wave; grp < ST_MGROUPS; grp += 4) {
        const int q = min(16 * grp + p, ST_MPIX - 1), my = q / ST_MCOLS, mx = q - my * ST_MCOLS;
        /* mid pixel (my, mx) is image pixel (y0 - 1 + my, x0 - 1 + mx); tap (ky, kx) of it is pixel (my + ky, mx + kx)
         * of the looked-up tile */
        const uint2* const b = s_x + my * ST_XCOLS + mx + 2 * g;
        hm_acc4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ky = 0; ky < ST_K0; ++ky) {
            const uint2 lo = b[ky * ST_XCOLS], hi = b[ky * ST_XCOLS + 1];
            /* kx = 7 is no tap: an exact zero, whatever pixel stands there */
            acc = hm_mfma<DT>(w0[ky], make_uint4(lo.x, lo.y, g == 3 ? 0u : hi.x, g == 3 ? 0u : hi.y), acc);
        }
        const int gy = y0 - 1 + my, gx = x0 - 1 + mx;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        uint32_t r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = inside ? hm_round<DT>(fmaxf(fmaf(sc0[i], acc[i], sh0[i]), 0.0f)) : 0u;
        if (16 * grp + p < ST_MPIX) {
            ((uint2*)s_mid)[2 * hm_slot(q, g >> 1) + (g & 1)] = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
            /* the workgroup that owns the pixel stores it */
            if (mid_out && inside && my >= 1 && my <= ST_ROWS && mx >= 1 && mx <= ST_COLS) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    mid_out[((size_t)n * 16 + 4 * g + i) * plane + (size_t)gy * W + gx] = (uint16_t)r[i];
            }
        }
    }
    __syncthreads();

    /* 4: out.  Step s of lane (p, g) is tap 2s + (g >> 1), channels 8 (g & 1) .. + 7; tap 9 is no tap. */
    int tap_at[ST_K1];
#pragma unroll
    for (int s = 0; s < ST_K1; ++s) {
        const int tap = min(2 * s + (g >> 1), 8);
        tap_at[s] = (tap / 3) * ST_MCOLS + tap % 3;
    }
    for (int grp = wave; grp < ST_OGROUPS; grp += 4) {
        const int row = grp / (ST_COLS / 16), col = (grp % (ST_COLS / 16)) * 16;
        const int at = row * ST_MCOLS + col + p;   /* tap (0, 0) of output pixel (row, col + p) in the mid tile */
        hm_acc4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < ST_K1; ++s) {
            uint4 a = s_mid[hm_slot(at + tap_at[s], g & 1)];
            if (s == ST_K1 - 1 && g >= 2) a = make_uint4(0, 0, 0, 0);
            acc = hm_mfma<DT>(a, w1[s], acc);
        }
        /* register i is pixel col + 4g + i of the row, channel p */
        const int y = y0 + row, x = x0 + col + 4 * g;
        uint32_t r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = hm_round<DT>(fmaxf(fmaf(sc1, acc[i], sh1), 0.0f));
        if (y < H && x < W) {
            uint16_t* const dst = out + ((size_t)n * 16 + p) * plane + (size_t)y * W + x;
            if (x + 3 < W) {
                /* four halves of a plane, aligned to the element alone: one 8-byte store */
                const uint2 v = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
                __builtin_memcpy(dst, &v, 8);
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (x + i < W) dst[i] = (uint16_t)r[i];
            }
        }
    }
}

/* The arguments are checked by is_stem_pack_weights. */
extern "C" hipError_t isk_launch_stem_pack(const float* d_w0, const float* d_w1, int dtype, void* d_packed, hipStream_t stream) {
    const dim3 grid(((ST_K0 + ST_K1) * 64 * 8 + 255) / 256);
    const bool half = hm_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_stem_pack<dt()>, grid, dim3(256), 0, stream, d_w0, d_w1, (uint16_t*)d_packed);
    });
    if (!half) return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" size_t isk_stem_packed_bytes(void) { return (size_t)(ST_K0 + ST_K1) * 64 * 16; }

/* The arguments are checked by is_core.hip's is_stem. */
extern "C" hipError_t isk_launch_stem(const is_stem_args* a, hipStream_t stream) {
    const int tiles_x = (a->cols + ST_COLS - 1) / ST_COLS, tiles_y = (a->rows + ST_ROWS - 1) / ST_ROWS;
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, a->n_images); /* at most 512 * 2048 by 65535 */
    const bool half = hm_dispatch(a->dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_stem<dt()>, grid, dim3(256), 0, stream, (const uint8_t*)a->d_image, (const uint16_t*)a->d_lut,
                           (const uint4*)a->d_packed, a->d_scale0, a->d_shift0, a->d_scale1, a->d_shift1,
                           (uint16_t*)a->d_mid, (uint16_t*)a->d_out, a->rows, a->cols, tiles_x);
    });
    if (!half) return hipErrorInvalidValue;
    return hipGetLastError();
}
