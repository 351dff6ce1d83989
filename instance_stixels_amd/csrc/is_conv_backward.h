/*
 * is_conv_backward.h -- what the backward kernels of f21 (is_k_conv_backward.hip), f22 (is_k_conv_backward_stride.hip)
 * and f23 (is_k_stem_backward.hip) share beyond is_half_mfma.h: the pieces of the weight-gradient kernels (all of them used
 * by k_conv_bwd_weight; k_conv_bwd_weight_s2 takes cb_decode and cb_clear and keeps its own staging, see its file), the
 * tap table of the stride-2 transposed convolution, and the host's scratch and grid helpers.
 *
 * The weight-gradient kernels k_conv_bwd_weight<DT, TAPS> (stride 1) and k_conv_bwd_weight_s2<DT, TAPS> are one implicit
 * GEMM with M = channels_out, N = channels_in x taps, K = the pixels of chunk (image, band of output rows).  Both
 * operands have K contiguous in memory (pixels of a row of an NCHW plane), which is the fragment of the 32x32x16 shapes
 * as it is (lane l: row l & 31, k = 8 (l >> 5) + j); neither needs a transpose.  For tap kx the x operand is shifted
 * against gh, so a fragment read straight from a row would start off 16-byte alignment.  That is solved in the staging:
 * per kx the workgroup holds its own copy of the x rows, in which pixel p of the segment is input column
 * STEP p + (kx - 1) d (stride 1: STEP = 1, the dilation d; stride 2: STEP = 2, d = 1: the copies deinterleave), so that
 * every fragment of every tap is one aligned ds_read_b128.
 *
 * Tile mapping.  A workgroup of four waves owns 64 co x 64 ci x all taps of one chunk; wave w takes the 32 x 32 block
 * (w & 1, w >> 1) with TAPS accumulators (144 registers at 3x3).  It walks segments of CB_SEG = 32 output pixels (two K
 * steps) of the chunk's rows.  A step (one output row y of one segment) multiplies the 4 KB tiles
 *   A         gh[co0 .. co0 + 63][y][xs .. xs + 31]
 *   B ky, kx  x[ci0 .. ci0 + 63][input row of (y, ky)][copy kx of xs .. xs + 31]
 * The x tiles are staged ONCE PER kx, not per tap: the three input rows of a step stay in a ring of three rows per kx
 * copy, and the kernel's schedule says which rows are new at a step and which ring slot holds the step's first row
 * (ky = 0); the rows of ky = 1, 2 are the next slots.  A pixel outside the image or past the row's end, and a channel
 * past the last, is zero (the address is clamped into the array and the loaded bits are masked: no select on a loaded
 * value).  Channels that are no multiple of 64 compute on zeros and are not stored.  Workgroup b is
 * taken to run on XCD b & 7 (the round-robin dispatch k_conv3x3 relies on): the weight tiles of ONE chunk follow each
 * other in that XCD's share of the grid, so that the chunk's gh and x can come from memory once and from that XCD's L2
 * for the other tiles.  Reasoned, not measured: the tiles of a chunk are 8 workgroups apart in the grid, and once more
 * workgroups than are resident lie between them they are not adjacent in time.
 *
 * LDS tile and its bank account (reasoned from the addresses, not measured).  A tile is [4 slots of 8 pixels][64 rows]
 * 16-byte entries; entry e(s, row) = 64 s + (row ^ 2 s).
 *   reads   ds_read_b128, lane (r, half) at K step ks reads entry e(2 ks + half, row0 + r).  A 16-lane group of that
 *           instruction holds 16 lanes of one half whose r are distinct mod 16 ({0-3, 12-15, 20-27}, {4-11, 16-19,
 *           28-31}); the XOR permutes inside an aligned group of 16 entries, so the group reads the 16 slots of one
 *           256-byte bank row: conflict-free.
 *   writes  ds_write_b32 of a pixel pair; a thread's item is (row, pair q), consecutive threads consecutive q.  Dword
 *           256 s + 4 (row ^ 2 s) + (q & 3) with s = q >> 2 (256 s is 0 mod the 32 banks): the 32 lanes of a half wave
 *           are rows 2 k and 2 k + 1 times 16 pairs; (row ^ 2 s) & 7 takes 8 distinct values over them, times 4
 *           dwords: 32 distinct banks of the 32 that a write sees: conflict-free.
 * The global loads are 2-byte loads (the row bases are only 2-byte aligned when the width is odd), consecutive lanes
 * consecutive pixels (at STEP = 2, 4 bytes apart: the three copies of a row read it 1.5 times, from the same cache
 * lines).  The loads of a step are issued one step ahead, raw, into registers and go to LDS between the two barriers of
 * their step, so they are in flight while the step before multiplies; a deeper pipeline is not built.
 */
#ifndef IS_CONV_BACKWARD_H_
#define IS_CONV_BACKWARD_H_
#include "is_half_mfma.h"

#define CB_SEG 32                  /* pixels of a staged segment: two K steps */
#define CB_TILE_ENTRIES 256        /* 16-byte entries of a 64-row x 32-pixel tile */

/* the LDS of a weight-gradient kernel: [1 + TAPS] tiles: gh, then x [ring slot][kx].  The launch's dynamic LDS: only
 * k_conv_bwd_weight and k_conv_bwd_weight_s2 are launched with any, and only they may name it. */
extern __shared__ uint4 cb_lds[];
/* entry of (slot s of 8 pixels, row) in a tile */
__device__ __forceinline__ int cb_entry(int s, int row) { return 64 * s + (row ^ (2 * s)); }

template <int N> __device__ __forceinline__ void cb_clear(hm_acc16 (&acc)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
}

/* A thread's four items (row, pixel pair q) of a tile are rows (tid >> 4) + 16 it, it = 0 .. 3, at pair tid & 15.
 * An operand as the thread sees it: the planes of its four rows, channels c0 + row of image n of p[n][C][H][W] halves
 * (a channel past the last: the last one's plane, masked when it goes to LDS). */
struct cb_planes {
    const uint16_t* ch[4];
    int c0, C, H, W;
};
__device__ __forceinline__ cb_planes cb_image(const uint16_t* p, int n, int c0, int C, int H, int W) {
    const size_t plane = (size_t)H * W;
    cb_planes g = {{}, c0, C, H, W};
#pragma unroll
    for (int it = 0; it < 4; ++it) g.ch[it] = p + ((size_t)n * C + min(c0 + ((int)threadIdx.x >> 4) + 16 * it, C - 1)) * plane;
    return g;
}

/* what a workgroup of the weight-gradient kernels owns: chunk (image n, output rows ya .. yb - 1), the 64 x 64 tile at
 * (co0, ci0), and in it the wave's 32 x 32 block at (mrow, nrow) */
struct cb_group {
    int chunk, n, ya, yb, co0, ci0, mrow, nrow;
};
/* workgroup b of the grid is taken to run on XCD b & 7: the weight tiles of a chunk follow each other there.
 * chunk >= chunks: the workgroup has nothing to do (the whole workgroup: return before any barrier) */
template <int BAND> __device__ __forceinline__ cb_group cb_decode(int rows_out, int bands, int tiles_ci, int tiles) {
    const int seq = blockIdx.x >> 3, tile = seq % tiles, wave = (int)threadIdx.x >> 6;
    cb_group g;
    g.chunk = (seq / tiles) * 8 + (blockIdx.x & 7);
    g.n = g.chunk / bands, g.ya = (g.chunk % bands) * BAND, g.yb = min(g.ya + BAND, rows_out);
    g.co0 = (tile / tiles_ci) * 64, g.ci0 = (tile % tiles_ci) * 64;
    g.mrow = 32 * (wave & 1), g.nrow = 32 * (wave >> 1);
    return g;
}

/* cb_load_*: the raw bits of a step, one step ahead, into registers; cb_store_*: the masks on the bits when the
 * registers go to LDS (no select on a loaded value).
 * A: row y of gh at channels c0 .. c0 + 63, pixels xs .. xs + 31. */
__device__ __forceinline__ void cb_load_a(uint32_t (&v)[4][2], const cb_planes& g, int y, int xs) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int p = xs + 2 * ((int)threadIdx.x & 15);
        const uint16_t* src = g.ch[it] + (size_t)y * g.W;
        v[it][0] = src[min(p, g.W - 1)], v[it][1] = src[min(p + 1, g.W - 1)];
    }
}
__device__ __forceinline__ void cb_store_a(const uint32_t (&v)[4][2], const cb_planes& g, int xs) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = (int)threadIdx.x + 256 * it, row = idx >> 4, q = idx & 15, p = xs + 2 * q;
        const bool in_c = g.c0 + row < g.C;
        uint32_t k0 = in_c && p < g.W ? 0xffffu : 0u, k1 = in_c && p + 1 < g.W ? 0xffffu : 0u;
        asm volatile("" : "+v"(k0), "+v"(k1)); /* a mask on the bits, not a branch around the loads */
        ((uint32_t*)cb_lds)[4 * cb_entry(q >> 2, row) + (q & 3)] = (v[it][0] & k0) | ((v[it][1] & k1) << 16);
    }
}
/* B: input row gy (any integer: outside the image it is zeros) of x at channels c0 .. c0 + 63 in its KX copies; the
 * pixel pair (p, p + 1) of copy kx is the input columns STEP p + (kx - 1) d and STEP more (KX = 1: d is 0).  Stored to
 * ring slot `slot`. */
template <int KX, int STEP>
__device__ __forceinline__ void cb_load_b(uint32_t (&v)[4][KX][2], const cb_planes& x, int gy, int xs, int d) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int p = xs + 2 * ((int)threadIdx.x & 15);
        const uint16_t* src = x.ch[it] + (size_t)min(max(gy, 0), x.H - 1) * x.W;
#pragma unroll
        for (int kx = 0; kx < KX; ++kx) {
            const int gx = STEP * p + (kx - 1) * d;
            v[it][kx][0] = src[min(max(gx, 0), x.W - 1)], v[it][kx][1] = src[min(max(gx + STEP, 0), x.W - 1)];
        }
    }
}
template <int KX, int STEP>
__device__ __forceinline__ void cb_store_b(int slot, const uint32_t (&v)[4][KX][2], const cb_planes& x, int gy, int xs, int d) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = (int)threadIdx.x + 256 * it, row = idx >> 4, q = idx & 15, p = xs + 2 * q;
        const bool in_y = x.c0 + row < x.C && gy >= 0 && gy < x.H;
#pragma unroll
        for (int kx = 0; kx < KX; ++kx) {
            const int gx = STEP * p + (kx - 1) * d;
            uint32_t k0 = in_y && gx >= 0 && gx < x.W ? 0xffffu : 0u, k1 = in_y && gx + STEP >= 0 && gx + STEP < x.W ? 0xffffu : 0u;
            asm volatile("" : "+v"(k0), "+v"(k1));
            ((uint32_t*)cb_lds)[4 * CB_TILE_ENTRIES * (1 + KX * slot + kx) + 4 * cb_entry(q >> 2, row) + (q & 3)] =
                (v[it][kx][0] & k0) | ((v[it][kx][1] & k1) << 16);
        }
    }
}

/* The MFMAs of a step on the LDS tiles into ACC[TAPS] for the cb_group G.  S0: the ring slot of the step's first input
 * row; tap (ky, kx) reads slot (S0 + ky) % 3, copy kx.  A macro: the same loop as a __forceinline__ function had the same
 * instruction counts but was scheduled 0.6 - 1.1 % slower at 512 channels (profiles/f24_multiply_bisect.log). */
#define CB_MULTIPLY(DT, TAPS, ACC, G, S0)                                                                            \
    do {                                                                                                             \
        const int cbm_s0 = (S0), cbm_r = (int)threadIdx.x & 31, cbm_half = ((int)threadIdx.x & 63) >> 5;             \
        _Pragma("unroll") for (int cbm_ks = 0; cbm_ks < CB_SEG / 16; ++cbm_ks) {                                     \
            const int cbm_s = 2 * cbm_ks + cbm_half;                                                                 \
            const uint4 cbm_a = cb_lds[cb_entry(cbm_s, (G).mrow + cbm_r)];                                           \
            const int cbm_eb = cb_entry(cbm_s, (G).nrow + cbm_r);                                                    \
            _Pragma("unroll") for (int cbm_t = 0; cbm_t < (TAPS); ++cbm_t) {                                         \
                const int cbm_tile = (TAPS) == 1 ? 1 : 1 + 3 * ((cbm_s0 + cbm_t / 3) % 3) + cbm_t % 3;               \
                (ACC)[cbm_t] = hm_mfma<DT>(cbm_a, cb_lds[CB_TILE_ENTRIES * cbm_tile + cbm_eb], (ACC)[cbm_t]);        \
            }                                                                                                        \
        }                                                                                                            \
    } while (0)

/* part[((chunk * TAPS + tap) * Cout + co) * Cin + ci]: k_conv_bwd_reduce's layout.  Register i of a lane is row
 * hm_cd_row(i, half) of the wave's block at column r: 32 lanes store 32 consecutive ci. */
template <int TAPS>
__device__ __forceinline__ void cb_store_part(float* part, const hm_acc16 (&acc)[TAPS], const cb_group& g, int Cout, int Cin) {
    const int lane = (int)threadIdx.x & 63, r = lane & 31, half = lane >> 5, ci = g.ci0 + g.nrow + r;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = g.co0 + g.mrow + hm_cd_row(i, half);
            if (co < Cout && ci < Cin) part[(((size_t)g.chunk * TAPS + tap) * Cout + co) * Cin + ci] = acc[tap][i];
        }
}

/* The 3x3 transposed convolution at stride 2 (dX of f22, g_out of f23).  dX[r][c] sums wT[tap] gh[y][x] over the taps
 * with 2 y + ky - 1 = r and 2 x + kx - 1 = c.  A CELL (Y, X) is the input pixels (2 Y + {0, 1}, 2 X + {0, 1}), one of
 * each parity class; its taps read gh at (Y .. Y + 1, X .. X + 1) only:
 *     class 0 (even, even)  tap 4 gh[Y][X]
 *     class 1 (even, odd)   tap 3 gh[Y][X + 1],  tap 5 gh[Y][X]
 *     class 2 (odd, even)   tap 1 gh[Y + 1][X],  tap 7 gh[Y][X]
 *     class 3 (odd, odd)    tap 0 gh[Y + 1][X + 1],  tap 2 gh[Y + 1][X],  tap 6 gh[Y][X + 1],  tap 8 gh[Y][X]
 * Tap (ky, kx) goes to class 2 (ky != 1) + (kx != 1) and reads b[2 (ky == 0) + (kx == 0)] of
 * b = {gh[Y][X], gh[Y][X + 1], gh[Y + 1][X], gh[Y + 1][X + 1]}.  One accumulator per class, the nine MFMAs in increasing
 * tap: the order is part of the "same bytes" contract.  w(tap): the weight fragment. */
template <int DT, class ACC, class W>
__device__ __forceinline__ void cb_parity_taps(ACC (&acc)[4], const uint4 (&b)[4], W&& w) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3, cls = 2 * (ky != 1) + (kx != 1);
        acc[cls] = hm_mfma<DT>(w(tap), b[2 * (ky == 0) + (kx == 0)], acc[cls]);
    }
}

/* ---- host ---- */
static inline size_t cb_align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
/* the bands of H OUTPUT rows: IS_CONV_BACKWARD_BAND rows at stride 1, IS_CONV_BACKWARD_STRIDE_BAND at stride 2 */
static inline int cb_bands(int H, int stride) {
    const int band = stride == 2 ? IS_CONV_BACKWARD_STRIDE_BAND : IS_CONV_BACKWARD_BAND;
    return (H + band - 1) / band;
}
/* The grid of a weight-gradient kernel over `bands` bands an image (0: it does not fit 31 bits), and its LDS. */
static inline long long cb_weight_grid(int n, int Cin, int Cout, int bands) {
    const long long tiles = (long long)((Cout + 63) / 64) * ((Cin + 63) / 64), chunks = (long long)n * bands;
    const long long grid = tiles * ((chunks + 7) / 8 * 8);
    return grid > 0x7fffffffLL ? 0 : grid;
}
static inline size_t cb_weight_lds(int taps) { return (size_t)(1 + taps) * CB_TILE_ENTRIES * 16; }

#endif /* IS_CONV_BACKWARD_H_ */
