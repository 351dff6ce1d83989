/*
 * is_k_stem_backward.hip -- f23: the backward pass of the stem (is_stem_backward): from dY, the gradient with respect
 * to layer1's output, to the gradients of layer0's and layer1's master weights, folded scales and shifts, with the masked
 * gradients gh1 and gh0 on the way.  Numerics contract: include/instance_stixels_core.h f23, DESIGN.md 10ac.
 *
 * k_stem_bwd_pack_t<DT>   the five B fragments of dMid's convolution, lane by lane as k_stem's blob holds layer1's:
 *   element (s * 64 + lane) * 8 + j is k = 32 s + 8 (lane >> 4) + j = 16 tap' + co of column ci = lane & 15:
 *   round(scale1[co] * w1_half[co][ci][8 - tap']), 0 where tap' = 9.
 *
 * k_stem_bwd_pack_next<DT>, k_stem_bwd_gout<DT>   source (b) only: g_out, the gradient with respect to layer1's output,
 *   from layer2's masked gradient (f22's dX at 16 input channels), rounded once to the half dtype into the scratch, where
 *   k_stem_bwd_data reads it as it reads dY.  Described at the kernels.  The fusion into k_stem_bwd_data (g_out staged
 *   in LDS and never stored) is not built: 64 bytes a pixel of traffic are its price.
 *
 * k_stem_bwd_data<DT>     is_k_stem.hip's tile: a workgroup of four waves owns SB_ROWS = 16 rows of SB_COLS = 64 pixels
 *   of one frame.
 *   1  gh1 on the tile plus a halo of 1, 18 x 66 pixels, into LDS as [pixel][16 channels] in k_stem's hm_slot layout
 *      (38 KB): a thread takes a pixel and eight channels, 8 + 8 two-byte loads of dY and out that consecutive lanes make
 *      at consecutive pixels, one 16-byte LDS write; a pixel outside the image is zero (the address is clamped into the
 *      image).  The owner of a pixel stores its gh1.
 *   2  the dshift1 tile sums from LDS in binary64.
 *   3  dMid exactly as k_stem's phase 4 computes out: pixels on M, five instructions, k = 16 tap' + co; a lane's four
 *      results are four consecutive pixels of ONE channel plane: masked by the stored mid, rounded, one 8-byte store of
 *      gh0; and the dshift0 tile sums.
 *   A halo gh1 pixel staged by two workgroups is the same rounding of the same two loads in both.
 *
 * k_stem_bwd_weight<DT>   one workgroup of four waves per chunk (image, band of SW_BAND rows, segment of SW_SEG columns).
 *   An implicit GEMM with pixels on K: M = co (16), N = 9 tiles of (tap, ci) for G1 and 10 tiles of 16 consecutive (ky,
 *   c, kx) of the 147 for G0 (the 13 slots past 147 are exact zeros and not stored), K = the chunk's pixels, a row of
 *   the chunk per step and two 32-pixel instructions per row.  Both operands have K contiguous in memory (pixels of a
 *   row), which is the fragment as it is; for tap kx the x operand is shifted against gh by kx - 1 (kx - 3) pixels, so
 *   the staging holds one copy of a row per kx (f21's answer): every fragment is one aligned ds_read_b128.  The rows of
 *   mid stay in a ring of 3 and the looked-up rows in a ring of 7, so a step stages gh1, gh0 and ONE new row of each:
 *   row r of mid lives in slot (r + 1) % 3, of x in slot (r + 3) % 7.  The 19 N-tiles are dealt to the waves (tile t to
 *   wave t & 3): an element has one accumulator.
 *   LDS rows are SW_SEG halves plus 8 of padding, 144 bytes: the 16 lanes of a ds_read_b128 group that read 16
 *   consecutive rows at one column then cover the 16 slots of a 256-byte bank row (144 r mod 256 takes the 16 multiples of
 *   16).  Reasoned from the addresses, not measured.
 */
#include "is_conv_backward.h"

#define SB_ROWS IS_STEM_BACKWARD_TILE_ROWS
#define SB_COLS IS_STEM_BACKWARD_TILE_COLS
#define SB_GROWS (SB_ROWS + 2)              /* gh1: a halo of 1 */
#define SB_GCOLS (SB_COLS + 2)
#define SB_GPIX (SB_GROWS * SB_GCOLS)
#define SB_OGROUPS (SB_ROWS * SB_COLS / 16)
#define SB_K1 5                             /* MFMA steps of dMid: k = 16 tap' + co, 144 padded to 160 */
#define SB_LDS_BYTES (SB_GPIX * 32 + 256 * 8)
static_assert(3 * SB_LDS_BYTES <= 160 * 1024, "gh1 and the sums fit the LDS three times a CU");
static_assert(SB_COLS % 16 == 0 && SB_OGROUPS % 4 == 0 && SB_ROWS == 16, "a group is 16 pixels of one row; four waves share them; a thread of the sums is (row, channel)");

#define SW_BAND IS_STEM_BACKWARD_BAND
#define SW_SEG IS_STEM_BACKWARD_SEGMENT
#define SW_RS (SW_SEG + 8)                  /* halves of an LDS row */
#define SW_ROW_GH 0                         /* [gh1, gh0][16 co] */
#define SW_ROW_MID 32                       /* [3 slots][3 kx][16 ci] */
#define SW_ROW_X (32 + 144)                 /* [7 slots][3 c][7 kx] */
#define SW_LDS_ROWS (32 + 144 + 147)
#define SW_TILES 19                         /* N-tiles: 9 of G1, 10 of G0 */
#define SW_LDS_BYTES (3 * 256 * 2 + SW_LDS_ROWS * SW_RS * 2)
static_assert(SW_SEG % 32 == 0 && (SW_RS * 2) % 16 == 0, "whole K steps; 16-byte aligned fragments");
static_assert(3 * SW_LDS_BYTES <= 160 * 1024 && SW_LDS_BYTES <= 65536, "three workgroups a CU");

template <int DT>
__global__ __launch_bounds__(256) void k_stem_bwd_pack_t(const float* __restrict__ w1, const float* __restrict__ scale1,
                                                         uint16_t* __restrict__ packed) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= SB_K1 * 64 * 8) return;
    const int j = e & 7, lane = (e >> 3) & 63, s = e >> 9, ci = lane & 15, g = lane >> 4;
    const int k = 32 * s + 8 * g + j, tap = k >> 4, co = k & 15;
    packed[e] = tap < 9 ? hm_scaled_weight<DT>(scale1[co], w1[(co * 16 + ci) * 9 + (8 - tap)]) : (uint16_t)0;
}

/* The A fragments of g_out, lane by lane: element ((chunk * 9 + tap) * 64 + lane) * 8 + j is
 * round(scale_next[co] * w_next_half[co][ci][tap]) with ci = lane & 15, co = 32 chunk + 8 (lane >> 4) + j. */
template <int DT>
__global__ __launch_bounds__(256) void k_stem_bwd_pack_next(const float* __restrict__ w, const float* __restrict__ scale,
                                                            uint16_t* __restrict__ packed, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = e & 7, lane = (e >> 3) & 63, tap = (e >> 9) % 9, chunk = (e >> 9) / 9;
    const int ci = lane & 15, co = 32 * chunk + 8 * (lane >> 4) + j;
    packed[e] = hm_scaled_weight<DT>(scale[co], w[((size_t)co * 16 + ci) * 9 + tap]);
}

/* g_out from the masked gradient of the stride-2 3x3 layer that reads `out` (f22's dX at 16 input channels).  A wave
 * owns 16 CELLS of one cell row: cell (Y, X) is the pixels (2 Y + {0, 1}, 2 X + {0, 1}), one of each parity class, and
 * its taps read gh at (Y .. Y + 1, X .. X + 1) only (is_conv_backward.h's cb_parity_taps).  Each class is its own
 * chain of 16x16x32 MFMAs, M = ci, N = the 16 cells, K = 32 co, in increasing 32-co chunk and, inside a chunk,
 * increasing tap: one accumulator per element.  The B fragment of a lane is 8 co of its cell's pixel: eight 2-byte
 * loads a pixel, which the 16 lanes of a group make at consecutive pixels of a plane; no LDS.  A gh pixel outside the
 * image is zero (address clamped, bits masked). */
template <int DT>
__global__ __launch_bounds__(256) void k_stem_bwd_gout(const uint16_t* __restrict__ gh, const uint4* __restrict__ packed,
                                                       uint16_t* __restrict__ gout, int Cn, int H, int W, int Ho, int Wo) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, g = lane >> 4;
    const int n = blockIdx.z, Y = blockIdx.y * 4 + wave, X = blockIdx.x * 16 + p;
    const size_t plane_o = (size_t)Ho * Wo, plane = (size_t)H * W;
    const uint16_t* const ghn = gh + (size_t)n * Cn * plane_o;
    const size_t at[4] = {(size_t)min(Y, Ho - 1) * Wo + min(X, Wo - 1), (size_t)min(Y, Ho - 1) * Wo + min(X + 1, Wo - 1),
                          (size_t)min(Y + 1, Ho - 1) * Wo + min(X, Wo - 1), (size_t)min(Y + 1, Ho - 1) * Wo + min(X + 1, Wo - 1)};
    const uint32_t keep[4] = {Y < Ho && X < Wo ? 0xffffu : 0u, Y < Ho && X + 1 < Wo ? 0xffffu : 0u,
                              Y + 1 < Ho && X < Wo ? 0xffffu : 0u, Y + 1 < Ho && X + 1 < Wo ? 0xffffu : 0u};
    hm_acc4 acc[4]; /* (even, even), (even, odd), (odd, even), (odd, odd) */
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = hm_acc4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int chunk = 0; chunk < Cn / 32; ++chunk) {
        const uint16_t* const base = ghn + (size_t)(32 * chunk + 8 * g) * plane_o;
        uint4 b[4]; /* gh[Y][X], gh[Y][X + 1], gh[Y + 1][X], gh[Y + 1][X + 1] */
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = base[j * plane_o + at[q]] & keep[q];
            b[q] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
        }
        const uint4* const wfrag = packed + (size_t)chunk * 9 * 64 + lane;
        cb_parity_taps<DT>(acc, b, [&](int t) { return wfrag[t * 64]; });
    }
    /* register i of a lane is ci = 4 g + i of cell X */
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int row = 2 * Y + (c >> 1), col = 2 * X + (c & 1);
        if (row >= H || col >= W) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) gout[((size_t)n * 16 + 4 * g + i) * plane + (size_t)row * W + col] = hm_round<DT>(acc[c][i]);
    }
}

/* The sum over r = 0 .. 15 of the 256 threads' values at [r][tid & 15], by threads 0 .. 15. */
__device__ __forceinline__ void sb_tile_sum(double v, double* lds, double* dst, size_t stride_co, bool want) {
    const int tid = threadIdx.x;
    __syncthreads(); /* (the previous use of lds is over) */
    lds[tid] = v;
    __syncthreads();
    if (want && tid < 16) {
        double s = 0.0;
        for (int r = 0; r < 16; ++r) s = s + lds[16 * r + tid];
        dst[(size_t)tid * stride_co] = s;
    }
}

/* shift_part[((n * 16 + co) * tiles + tile] */
template <int DT>
__global__ __launch_bounds__(256) void k_stem_bwd_data(const void* __restrict__ dy_, int dy_f32, long long dy_stride,
                                                       const uint16_t* __restrict__ out, const uint16_t* __restrict__ mid,
                                                       const uint4* __restrict__ packed, uint16_t* __restrict__ gh1_out,
                                                       uint16_t* __restrict__ gh0_out, double* __restrict__ shift1_part,
                                                       double* __restrict__ shift0_part, int H, int W, int tiles_x) {
    __shared__ uint4 s_gh[2 * SB_GPIX];   /* hm_slot(pixel of the gh1 tile, channel half) */
    __shared__ double s_sum[256];
    static_assert(sizeof(s_gh) + sizeof(s_sum) == SB_LDS_BYTES, "the LDS account of the header");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, g = lane >> 4;
    const int n = blockIdx.y, y0 = (blockIdx.x / tiles_x) * SB_ROWS, x0 = (blockIdx.x % tiles_x) * SB_COLS;
    const size_t plane = (size_t)H * W, tiles = gridDim.x;
    const uint16_t* const outn = out + (size_t)n * 16 * plane;
    const uint16_t* const midn = mid + (size_t)n * 16 * plane;
    const size_t dyn = (size_t)n * (size_t)dy_stride;

    uint4 wt[SB_K1];
#pragma unroll
    for (int s = 0; s < SB_K1; ++s) wt[s] = packed[s * 64 + lane];

    /* 1: gh1 on the tile plus a halo of 1 */
    for (int it = tid; it < 2 * SB_GPIX; it += 256) {
        const int h = it >= SB_GPIX, q = it - h * SB_GPIX, qy = q / SB_GCOLS, qx = q - qy * SB_GCOLS;
        const int gy = y0 - 1 + qy, gx = x0 - 1 + qx;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t at = (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
        uint32_t r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t e = (size_t)(8 * h + j) * plane + at;
            const float o = hm_widen<DT>(outn[e]);
            const float gv = dy_f32 ? ((const float*)dy_)[dyn + e] : hm_widen<DT>(((const uint16_t*)dy_)[dyn + e]);
            r[j] = inside && o > 0.0f ? hm_round<DT>(gv) : 0u;
        }
        s_gh[hm_slot(q, h)] = make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
        /* the workgroup that owns the pixel stores it */
        if (inside && qy >= 1 && qy <= SB_ROWS && qx >= 1 && qx <= SB_COLS) {
#pragma unroll
            for (int j = 0; j < 8; ++j) gh1_out[((size_t)n * 16 + 8 * h + j) * plane + at] = (uint16_t)r[j];
        }
    }
    __syncthreads();

    /* 2: the dshift1 sums of the tile: thread (row tid >> 4, channel tid & 15), increasing column; the halo is not
     * part of it, a pixel outside the image is +0 */
    {
        const int c = tid & 15, row = tid >> 4;
        double s = 0.0;
        if (shift1_part) {
            for (int x = 0; x < SB_COLS; ++x) {
                const int q = (row + 1) * SB_GCOLS + x + 1;
                s = s + (double)hm_widen<DT>(((const uint16_t*)s_gh)[8 * hm_slot(q, c >> 3) + (c & 7)]);
            }
        }
        sb_tile_sum(s, s_sum, shift1_part + ((size_t)n * 16) * tiles + blockIdx.x, tiles, shift1_part != nullptr);
    }

    /* 3: dMid and gh0.  Step s of lane (p, g) is tap' 2s + (g >> 1), channels 8 (g & 1) .. + 7; tap' 9 is no tap. */
    int tap_at[SB_K1];
#pragma unroll
    for (int s = 0; s < SB_K1; ++s) {
        const int tap = min(2 * s + (g >> 1), 8);
        tap_at[s] = (tap / 3) * SB_GCOLS + tap % 3;
    }
    double sum0 = 0.0;
    for (int grp = wave; grp < SB_OGROUPS; grp += 4) {
        const int row = grp / (SB_COLS / 16), col = (grp % (SB_COLS / 16)) * 16;
        const int at = row * SB_GCOLS + col + p;   /* tap' (0, 0) of pixel (row, col + p) in the gh1 tile */
        hm_acc4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < SB_K1; ++s) {
            uint4 a = s_gh[hm_slot(at + tap_at[s], g & 1)];
            if (s == SB_K1 - 1 && g >= 2) a = make_uint4(0, 0, 0, 0);
            acc = hm_mfma<DT>(a, wt[s], acc);
        }
        /* register i is pixel col + 4g + i of the row, channel p */
        const int y = y0 + row, x = x0 + col + 4 * g;
        uint32_t r[4] = {0u, 0u, 0u, 0u};
        if (y < H && x < W) {
            const size_t e = ((size_t)n * 16 + p) * plane + (size_t)y * W + x;
            uint16_t m[4] = {0, 0, 0, 0};
            if (x + 3 < W) {
                __builtin_memcpy(m, midn + ((size_t)p * plane + (size_t)y * W + x), 8);
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (x + i < W) m[i] = midn[(size_t)p * plane + (size_t)y * W + x + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = x + i < W && hm_widen<DT>(m[i]) > 0.0f ? hm_round<DT>(acc[i]) : 0u;
            if (x + 3 < W) {
                const uint2 v = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
                __builtin_memcpy(gh0_out + e, &v, 8);
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (x + i < W) gh0_out[e + i] = (uint16_t)r[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) sum0 = sum0 + (double)hm_widen<DT>((uint16_t)r[i]);
    }
    /* thread tid holds channel tid & 15: the same sum over tid >> 4 = 4 wave + g */
    sb_tile_sum(sum0, s_sum, shift0_part + ((size_t)n * 16) * tiles + blockIdx.x, tiles, shift0_part != nullptr);
}

/* part1[(chunk * 9 + tap) * 256 + co * 16 + ci], part0[(chunk * 49 + tap) * 48 + co * 3 + c]: k_conv_bwd_reduce's layout;
 * chunk = (image * bands + band) * segs + segment */
template <int DT>
__global__ __launch_bounds__(256) void k_stem_bwd_weight(const uint8_t* __restrict__ image, const uint16_t* __restrict__ lut,
                                                         const uint16_t* __restrict__ mid, const uint16_t* __restrict__ gh1,
                                                         const uint16_t* __restrict__ gh0, float* __restrict__ part1,
                                                         float* __restrict__ part0, int H, int W, int segs) {
    __shared__ uint16_t s_lut[3 * 256];
    __shared__ uint4 s_rows4[SW_LDS_ROWS * SW_RS / 8];
    static_assert(sizeof(s_lut) + sizeof(s_rows4) == SW_LDS_BYTES, "the LDS account of the header");
    uint16_t* const s_rows = (uint16_t*)s_rows4;
    uint32_t* const s_pairs = (uint32_t*)s_rows4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, g = lane >> 4;
    const int n = blockIdx.y, band = blockIdx.x / segs, seg = blockIdx.x - band * segs;
    const int ya = band * SW_BAND, yb = min(ya + SW_BAND, H), xs = seg * SW_SEG;
    const size_t plane = (size_t)H * W;
    const uint8_t* const img = image + (size_t)n * plane * 3;
    const uint16_t* const midn = mid + (size_t)n * 16 * plane;
    const uint16_t* const gh1n = gh1 + (size_t)n * 16 * plane;
    const uint16_t* const gh0n = gh0 + (size_t)n * 16 * plane;

    for (int i = tid; i < 3 * 256; i += 256) s_lut[i] = lut[i];

    /* the lane's column of each of the wave's tiles t = wave + 4 i: the row of its A operand, and of its B operand
     * (the ring slot of row y + ky, then kx and the channel), or no column at all (G0's slots past 147) */
    int a_row[5], b_ky[5], b_inner[5];
    bool live[5], is_g1[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int t = wave + 4 * i;
        if (t < 9) { /* G1, tap t: column ci = p */
            a_row[i] = SW_ROW_GH + p, b_ky[i] = t / 3, b_inner[i] = (t % 3) * 16 + p, live[i] = true, is_g1[i] = true;
        } else {     /* G0: column idx = 16 (t - 9) + p = (ky * 3 + c) * 7 + kx */
            const int idx = min(16 * (t - 9) + p, 146);
            a_row[i] = SW_ROW_GH + 16 + p, b_ky[i] = idx / 21, b_inner[i] = idx % 21, is_g1[i] = false;
            live[i] = t < SW_TILES && 16 * (t - 9) + p < 147;
        }
    }
    hm_acc4 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = hm_acc4{0.0f, 0.0f, 0.0f, 0.0f};

    /* A pixel pair of a row, from `src` (a row of a plane, or null for a row outside the image) shifted by `shift`
     * pixels: the address is clamped into the row and the bits are masked. */
    auto pair_of = [&](const uint16_t* src, bool in_y, int q, int shift) -> uint32_t {
        const int gx = xs + 2 * q + shift;
        const uint32_t v0 = src[min(max(gx, 0), W - 1)], v1 = src[min(max(gx + 1, 0), W - 1)];
        const uint32_t k0 = in_y && gx >= 0 && gx < W ? 0xffffu : 0u, k1 = in_y && gx + 1 >= 0 && gx + 1 < W ? 0xffffu : 0u;
        return (v0 & k0) | ((v1 & k1) << 16);
    };
    /* row r of mid in its three kx copies */
    auto stage_mid = [&](int r) {
        const bool in_y = r >= 0 && r < H;
        const int slot = (r + 1) % 3;
        const uint16_t* const base = midn + (size_t)min(max(r, 0), H - 1) * W;
        for (int it = tid; it < 3 * 16 * (SW_SEG / 2); it += 256) {
            const int q = it % (SW_SEG / 2), ci = (it / (SW_SEG / 2)) & 15, kx = it / (16 * (SW_SEG / 2));
            s_pairs[(SW_ROW_MID + (slot * 3 + kx) * 16 + ci) * (SW_RS / 2) + q] = pair_of(base + (size_t)ci * plane, in_y, q, kx - 1);
        }
    };
    /* row r of the looked-up image in its seven kx copies, three channels each */
    auto stage_x = [&](int r) {
        const bool in_y = r >= 0 && r < H;
        const int slot = (r + 3) % 7;
        const uint8_t* const base = img + (size_t)min(max(r, 0), H - 1) * W * 3;
        for (int it = tid; it < 7 * (SW_SEG / 2); it += 256) {
            const int q = it % (SW_SEG / 2), kx = it / (SW_SEG / 2), gx = xs + 2 * q + kx - 3;
            const uint8_t* const b0 = base + (size_t)min(max(gx, 0), W - 1) * 3;
            const uint8_t* const b1 = base + (size_t)min(max(gx + 1, 0), W - 1) * 3;
            const uint32_t k0 = in_y && gx >= 0 && gx < W ? 0xffffu : 0u, k1 = in_y && gx + 1 >= 0 && gx + 1 < W ? 0xffffu : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t v0 = s_lut[256 * c + b0[c]], v1 = s_lut[256 * c + b1[c]];
                s_pairs[(SW_ROW_X + (slot * 3 + c) * 7 + kx) * (SW_RS / 2) + q] = (v0 & k0) | ((v1 & k1) << 16);
            }
        }
    };
    auto stage_gh = [&](int y) {
        for (int it = tid; it < 2 * 16 * (SW_SEG / 2); it += 256) {
            const int q = it % (SW_SEG / 2), row = it / (SW_SEG / 2);
            const uint16_t* const src = (row < 16 ? gh1n : gh0n) + (size_t)(row & 15) * plane + (size_t)y * W;
            s_pairs[(SW_ROW_GH + row) * (SW_RS / 2) + q] = pair_of(src, true, q, 0);
        }
    };

    __syncthreads(); /* the table */
    stage_mid(ya - 1), stage_mid(ya);
    for (int r = ya - 3; r < ya + 3; ++r) stage_x(r);
    for (int y = ya; y < yb; ++y) {
        if (y > ya) __syncthreads(); /* the previous step's operands are no longer read */
        stage_gh(y), stage_mid(y + 1), stage_x(y + 3);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < SW_SEG / 32; ++ks) {
            const int at = 32 * ks + 8 * g;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (wave + 4 * i >= SW_TILES) continue; /* (wave-uniform) */
                const uint4 a = *(const uint4*)(s_rows + a_row[i] * SW_RS + at);
                const int row = (is_g1[i] ? SW_ROW_MID + ((y + b_ky[i]) % 3) * 48 : SW_ROW_X + ((y + b_ky[i]) % 7) * 21) + b_inner[i];
                uint4 b = *(const uint4*)(s_rows + row * SW_RS + at);
                if (!live[i]) b = make_uint4(0, 0, 0, 0);
                acc[i] = hm_mfma<DT>(a, b, acc[i]);
            }
        }
    }

    /* register r of a lane is co = 4 g + r at the lane's column */
    const size_t chunk = ((size_t)n * gridDim.x) + blockIdx.x;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int t = wave + 4 * i;
        if (t >= SW_TILES || !live[i]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = 4 * g + r;
            if (t < 9) {
                part1[(chunk * 9 + t) * 256 + co * 16 + p] = acc[i][r];
            } else {
                const int idx = 16 * (t - 9) + p, ky = idx / 21, c = (idx % 21) / 7, kx = idx % 7;
                part0[(chunk * 49 + ky * 7 + kx) * 48 + co * 3 + c] = acc[i][r];
            }
        }
    }
}

static int sb_tiles(int H, int W) { return ((H + SB_ROWS - 1) / SB_ROWS) * ((W + SB_COLS - 1) / SB_COLS); }
static int sb_chunks(int H, int W) { return ((H + SW_BAND - 1) / SW_BAND) * ((W + SW_SEG - 1) / SW_SEG); }

/* the sections of the scratch, in this order, each 16-byte aligned */
struct sb_scratch {
    size_t gh1, gh0, packed, shift1, shift0, gsum1, gsum0, part1, part0, gout, packed_next, end;
};
static sb_scratch sb_layout(int n, int H, int W, int Cn) {
    const size_t P = (size_t)H * W, tiles = sb_tiles(H, W), chunks = (size_t)n * sb_chunks(H, W);
    sb_scratch s;
    s.gh1 = 0;
    s.gh0 = s.gh1 + cb_align16((size_t)n * 16 * P * 2);
    s.packed = s.gh0 + cb_align16((size_t)n * 16 * P * 2);
    s.shift1 = s.packed + cb_align16((size_t)SB_K1 * 64 * 16);
    s.shift0 = s.shift1 + cb_align16((size_t)n * 16 * tiles * 8);
    s.gsum1 = s.shift0 + cb_align16((size_t)n * 16 * tiles * 8);
    s.gsum0 = s.gsum1 + cb_align16((size_t)16 * 16 * 9 * 8);
    s.part1 = s.gsum0 + cb_align16((size_t)16 * 3 * 49 * 8);
    s.part0 = s.part1 + cb_align16(chunks * 16 * 16 * 9 * 4);
    s.gout = s.part0 + cb_align16(chunks * 16 * 3 * 49 * 4);
    s.packed_next = s.gout + (Cn ? cb_align16((size_t)n * 16 * P * 2) : 0);
    s.end = s.packed_next + cb_align16((size_t)(Cn / 32) * 9 * 64 * 16);
    return s;
}

/* The arguments are checked by is_core.hip's stem_backward_shape_fault.  0: a grid does not fit (n_images * chunks
 * beyond 31 bits cannot happen below 65535 * 1024 * 512, so only the launch's own limits count). */
extern "C" size_t isk_stem_backward_scratch_bytes(int n_images, int rows, int cols, int channels_next) {
    return sb_layout(n_images, rows, cols, channels_next).end;
}

/* The arguments are checked by is_core.hip's is_stem_backward. */
extern "C" hipError_t isk_launch_stem_backward(const is_stem_backward_args* a, hipStream_t stream) {
    const int n = a->n_images, H = a->rows, W = a->cols;
    const int tiles_x = (W + SB_COLS - 1) / SB_COLS, tiles = sb_tiles(H, W);
    const int segs = (W + SW_SEG - 1) / SW_SEG, chunks_image = sb_chunks(H, W), chunks = n * chunks_image;
    const int Cn = a->d_grad_next ? a->channels_next : 0;
    const sb_scratch lay = sb_layout(n, H, W, Cn);
    char* const scratch = (char*)a->d_scratch;
    uint16_t* const gh1 = a->d_grad_pre1 ? (uint16_t*)a->d_grad_pre1 : (uint16_t*)(scratch + lay.gh1);
    uint16_t* const gh0 = a->d_grad_pre0 ? (uint16_t*)a->d_grad_pre0 : (uint16_t*)(scratch + lay.gh0);
    uint16_t* const packed = (uint16_t*)(scratch + lay.packed);
    double* const shift1 = (double*)(scratch + lay.shift1);
    double* const shift0 = (double*)(scratch + lay.shift0);
    double* const gsum1 = (double*)(scratch + lay.gsum1);
    double* const gsum0 = (double*)(scratch + lay.gsum0);
    float* const part1 = (float*)(scratch + lay.part1);
    float* const part0 = (float*)(scratch + lay.part0);
    if (a->dtype != IS_HEAD_F16 && a->dtype != IS_HEAD_BF16) return hipErrorInvalidValue;
    const bool contract = a->d_grad_weight0 || a->d_grad_scale0 || a->d_grad_weight1 || a->d_grad_scale1;
    /* the gradient with respect to out: dY, or g_out computed into the scratch in the half dtype */
    const void* dy = a->d_grad_out;
    int dy_f32 = a->grad_out_dtype == IS_HEAD_F32;
    long long dy_stride = a->grad_image_stride;

    hm_dispatch(a->dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_stem_bwd_pack_t<dt()>, dim3((SB_K1 * 64 * 8 + 255) / 256), dim3(256), 0, stream, a->d_w1,
                           a->d_scale1, packed);
    });
    if (Cn) {
        uint16_t* const gout = (uint16_t*)(scratch + lay.gout);
        uint16_t* const packed_next = (uint16_t*)(scratch + lay.packed_next);
        const int total = (Cn / 32) * 9 * 512, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
        const dim3 grid((Wo + 15) / 16, (Ho + 3) / 4, n);
        hm_dispatch(a->dtype, [&](auto dt) {
            hipLaunchKernelGGL(k_stem_bwd_pack_next<dt()>, dim3((total + 255) / 256), dim3(256), 0, stream,
                               a->d_weight_next, a->d_scale_next, packed_next, total);
        });
        hm_dispatch(a->dtype, [&](auto dt) {
            hipLaunchKernelGGL(k_stem_bwd_gout<dt()>, grid, dim3(256), 0, stream, (const uint16_t*)a->d_grad_next,
                               (const uint4*)packed_next, gout, Cn, H, W, Ho, Wo);
        });
        dy = gout, dy_f32 = 0, dy_stride = 16LL * H * W;
    }
    hm_dispatch(a->dtype, [&](auto dt) {
        const dim3 grid((unsigned)tiles, n); /* at most 512 * 2048 by 65535 */
        double* const sp1 = a->d_grad_shift1 ? shift1 : nullptr;
        double* const sp0 = a->d_grad_shift0 ? shift0 : nullptr;
        hipLaunchKernelGGL(k_stem_bwd_data<dt()>, grid, dim3(256), 0, stream, dy, dy_f32, dy_stride, (const uint16_t*)a->d_out,
                           (const uint16_t*)a->d_mid, (const uint4*)packed, gh1, gh0, sp1, sp0, H, W, tiles_x);
    });
    if (contract) hm_dispatch(a->dtype, [&](auto dt) {
        const dim3 grid((unsigned)chunks_image, n); /* at most 1024 * 512 by 65535 */
        hipLaunchKernelGGL(k_stem_bwd_weight<dt()>, grid, dim3(256), 0, stream, (const uint8_t*)a->d_image,
                           (const uint16_t*)a->d_lut, (const uint16_t*)a->d_mid, (const uint16_t*)gh1, (const uint16_t*)gh0,
                           part1, part0, H, W, segs);
    });
    if (a->d_grad_weight1 || a->d_grad_scale1)
        isk_launch_conv_bwd_reduce(part1, chunks, 16, 16, 9, a->d_scale1, a->d_grad_weight1, a->d_grad_scale1 ? gsum1 : nullptr, stream);
    if (a->d_grad_weight0 || a->d_grad_scale0)
        isk_launch_conv_bwd_reduce(part0, chunks, 3, 16, 49, a->d_scale0, a->d_grad_weight0, a->d_grad_scale0 ? gsum0 : nullptr, stream);
    if (a->d_grad_scale1 || a->d_grad_shift1)
        isk_launch_conv_bwd_channel(a->dtype, gsum1, a->d_w1, shift1, n, tiles, 16, 16, 9, a->d_grad_scale1, a->d_grad_shift1, stream);
    if (a->d_grad_scale0 || a->d_grad_shift0)
        isk_launch_conv_bwd_channel(a->dtype, gsum0, a->d_w0, shift0, n, tiles, 3, 16, 49, a->d_grad_scale0, a->d_grad_shift0, stream);
    return hipGetLastError();
}
